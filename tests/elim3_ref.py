"""Reference side of the Pose3 elimination (TEST INFRASTRUCTURE, not collected): ROME_BLOCKOP_COMPOSE on Pose3 blocks (inversion flags,
star-mesh inflation), ROME_BLOCKOP_ANCHOR_MEAN, and the sampled-measurement Pose3Pose3 rows of an up-solve plan.

Three statements of the same formulas:
  * float64 NumPy (`compose3`, `inflate3`, `anchor_mean3`): store coordinates (t, ω), q = Exp(ω); inverse (−R(q)ᵀ t, conj q); composition
    (t_a + R(q_a) t_b, q_a ⊗ q_b); stored as Log of the w >= 0 representative with the library's θ = π snap (2 q_w² <= √eps -> θ = π
    exactly).  Means: mean translation, q_m = q_0 ⊗ Exp(mean_i Log(conj q_0 ⊗ q_i)); sums in the kernel's order (lane partials of 256
    lanes, then the halving tree).  Inflation about the mean of the block AS STORED: t' = t_m + g_t (t − t_m),
    q' = q_m ⊗ Exp(g_θ Log(conj q_m ⊗ q)).
  * mpmath at lin_ref.DPS digits (`mp_compose3`, `mp_mean3`, `mp_inflate3`): the same, unrounded, results as group elements (t, q);
    no snap (the snap zone is compared by its own rule, as tests/conv_ref.py does).
  * the oracle backend of the solver (`Elim3Backend`): tests/dist_standin.py's OracleTreeBackend with the two block operations above and
    with an up-solve restatement for levels of Pose3 variables that hands the samples of a SampledPose3Pose3 row to the oracle's
    conv_pose3pose3 as `noise` with mu = 0, L = I (tests/solve_ref.py's upsolve_ref does that for the Pose2 families only).

`reference(N)`: the shared case table of the block-operation tests with its float64 and mp results, the measured deviations and the
bounds (rule of tests/test_gpu_device_math.py: per output block, bound = max(8 dev, 64 ulp) x scale)."""
import functools
import math

import mpmath as mpm
import numpy as np

import conv_ref as CR
from conv_ref import q_conj, q_exp, q_mul, q_rot
from dist_standin import OracleTreeBackend, OracleTreeBlockOp, OracleTreePlan
from lin_ref import DPS, EPS, SQRT_EPS

LANES = 256


# ------------------------------------------------------------------------------------------------------------ float64
def q_log_snap(q):
    """Log of the w >= 0 representative; θ = π exactly where 2 q_w² <= √eps (rome_device_math.hpp quat_log)"""
    w = CR.q_log(q)
    n = np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1))
    zone = 2.0 * q[..., 0] ** 2 <= SQRT_EPS
    k = np.where(q[..., 0] < 0.0, -1.0, 1.0) * math.pi / np.where(zone, n, 1.0)
    return np.where(zone[..., None], k[..., None] * q[..., 1:], w)


def load3(P):
    """(6, N) block -> t (N, 3), q (N, 4)"""
    return np.ascontiguousarray(P[:3].T), q_exp(np.ascontiguousarray(P[3:].T))


def invert3(t, q):
    qc = q_conj(q)
    return -q_rot(qc, t), qc


def compose3(A, B, inv_a=False, inv_b=False):
    ta, qa = load3(A); tb, qb = load3(B)
    if inv_a:
        ta, qa = invert3(ta, qa)
    if inv_b:
        tb, qb = invert3(tb, qb)
    return np.concatenate([(ta + q_rot(qa, tb)).T, q_log_snap(q_mul(qa, qb)).T])


def block_sum(x):
    """(N, k) -> (k,): partial sums of lanes i, i + 256, ... in order, then the halving tree over the 256 lanes"""
    N, k = x.shape
    xp = np.concatenate([x, np.zeros(((-N) % LANES, k))]).reshape(-1, LANES, k)
    acc = np.zeros((LANES, k))
    for r in xp:
        acc = acc + r
    w = LANES // 2
    while w:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w >>= 1
    return acc[0]


def mean3(P):
    """-> (t_m (3,), q_m (4,))"""
    t, q = load3(P)
    N = len(t)
    d = q_log_snap(q_mul(q_conj(q[:1]), q))
    s = block_sum(np.concatenate([t, d], axis=1)) * (1.0 / N)
    return s[:3], q_mul(q[0], q_exp(s[3:]))


def anchor_mean3(P):
    tm, qm = mean3(P)
    return np.repeat(np.concatenate([tm, q_log_snap(qm)])[:, None], P.shape[1], axis=1)


def inflate3(D, gt, gth):
    if gt == 1.0 and gth == 1.0:
        return D.copy()
    tm, qm = mean3(D)
    t, q = load3(D)
    d = q_log_snap(q_mul(q_conj(qm[None]), q))
    qn = q_mul(qm[None], q_exp(gth * d))
    return np.concatenate([(tm + gt * (t - tm)).T, q_log_snap(qn).T])


# ------------------------------------------------------------------------------------------------------------ mpmath
def _f(v):
    return mpm.mpf(float(v))


def mq_exp(w):
    th = mpm.sqrt(sum(v * v for v in w))
    if th == 0:
        return [mpm.mpf(1), mpm.mpf(0), mpm.mpf(0), mpm.mpf(0)]
    k = mpm.sin(th / 2) / th
    return [mpm.cos(th / 2)] + [k * v for v in w]


def mq_mul(p, q):
    return [p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
            p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]]


def mq_conj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def mq_rot(q, v):
    r = mq_mul(mq_mul(q, [mpm.mpf(0)] + list(v)), mq_conj(q))
    return r[1:]


def mq_log(q):
    """principal rotation vector of ±q"""
    n = mpm.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if n == 0:
        return [mpm.mpf(0)] * 3
    k = 2 * mpm.atan2(n, abs(q[0])) / n
    if q[0] < 0:
        k = -k
    return [k * v for v in q[1:]]


def mq_angle(q):
    return 2 * mpm.atan2(mpm.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), abs(q[0]))


def mp_load3(P, i):
    return [_f(P[k, i]) for k in range(3)], mq_exp([_f(P[3 + k, i]) for k in range(3)])


def mp_invert3(t, q):
    qc = mq_conj(q)
    return [-v for v in mq_rot(qc, t)], qc


def mp_compose3(A, B, i, inv_a=False, inv_b=False):
    """particle i -> (t, q)"""
    ta, qa = mp_load3(A, i); tb, qb = mp_load3(B, i)
    if inv_a:
        ta, qa = mp_invert3(ta, qa)
    if inv_b:
        tb, qb = mp_invert3(tb, qb)
    r = mq_rot(qa, tb)
    return [ta[k] + r[k] for k in range(3)], mq_mul(qa, qb)


def mp_mean3(P):
    N = P.shape[1]
    t0, q0 = mp_load3(P, 0)
    st, sd = [mpm.mpf(0)] * 3, [mpm.mpf(0)] * 3
    for i in range(N):
        t, q = mp_load3(P, i)
        d = mq_log(mq_mul(mq_conj(q0), q))
        st = [a + b for a, b in zip(st, t)]; sd = [a + b for a, b in zip(sd, d)]
    return [v / N for v in st], mq_mul(q0, mq_exp([v / N for v in sd]))


def mp_inflate3(D, idx, gt, gth):
    """particles idx of the float64 block D (the composition as stored) inflated about D's mean -> [(t, q)]"""
    tm, qm = mp_mean3(D)
    out = []
    for i in idx:
        t, q = mp_load3(D, i)
        d = mq_log(mq_mul(mq_conj(qm), q))
        out.append(([tm[k] + _f(gt) * (t[k] - tm[k]) for k in range(3)], mq_mul(qm, mq_exp([_f(gth) * v for v in d]))))
    return out


def mp_distance(coords, el):
    """six float64 store coordinates against an mp element (t, q) -> (translation error, rotation angle of q_refᵀ q), floats"""
    t, q = el
    et = max(abs(_f(coords[k]) - t[k]) for k in range(3))
    er = mq_angle(mq_mul(mq_conj(q), mq_exp([_f(coords[3 + k]) for k in range(3)])))
    return float(et), float(er)


def np_distance(X, Y):
    """(6, N) blocks as group elements -> (translation error (N,), rotation angle (N,))"""
    tx, qx = load3(X); ty, qy = load3(Y)
    return np.abs(tx - ty).max(axis=1), CR.q_angle(q_mul(q_conj(qy), qx))


# ------------------------------------------------------------------------------------------------------------ the case table
FLAGS = ((False, False), (True, False), (False, True), (True, True))
ZONE_MAGS = tuple(m for m in CR.P3_MAGS if 0.0 < math.pi - m < CR.ZONE_EDGE)


def _belief(rng, N, mean, st, sr):
    """N particles mean ⊕ (st ξ, sr ξ): (6, N)"""
    M = np.repeat(np.asarray(mean, dtype=float)[:, None], N, axis=1)
    E = np.concatenate([st * rng.standard_normal((3, N)), sr * rng.standard_normal((3, N))])
    return compose3(M, E)


def cases(N):
    """-> list of dict(A, B, flags, prm, kind).  kind "edge": every particle's composition has the rotation angle `mag` about the particle's own
    axis (A' = Exp(u α), B' = Exp(u (mag − α))), the SE(3) magnitudes of conv_ref.P3_MAGS -- the two inside the snap zone at translation scale 1
    only, which keeps the zone's share of the table under 5 %; "axis": common-axis compositions 2 + 2 > π; "random"; "belief": two beliefs
    composed, with and without inflation."""
    rng = np.random.default_rng(1000 + N)
    out = []

    def axis_pair(alpha, beta, fl, s):
        u = CR._unit(rng, (N,))
        wa = (-1.0 if fl[0] else 1.0) * alpha[:, None] * u
        wb = (-1.0 if fl[1] else 1.0) * beta[:, None] * u
        A = np.concatenate([s * rng.standard_normal((3, N)), wa.T]); B = np.concatenate([s * rng.standard_normal((3, N)), wb.T])
        return A, B
    k = 0
    for s in (1.0, 100.0):
        for mag in CR.P3_MAGS:
            if s != 1.0 and mag in ZONE_MAGS:
                continue
            fl = FLAGS[k % 4]; k += 1
            al = rng.uniform(0.3, 1.5, N)
            A, B = axis_pair(al, mag - al, fl, s)
            out.append(dict(A=A, B=B, flags=fl, prm=(1.0, 1.0), kind="edge", scale=s))
        for fl in FLAGS:
            A, B = axis_pair(np.full(N, 2.0), np.full(N, 2.0), fl, s)
            out.append(dict(A=A, B=B, flags=fl, prm=(1.0, 1.0), kind="axis", scale=s))
        for fl in FLAGS:
            A = np.concatenate([s * rng.standard_normal((3, N)), (CR._unit(rng, (N,)) * rng.uniform(0, 1.3, (N, 1))).T])
            B = np.concatenate([s * rng.standard_normal((3, N)), (CR._unit(rng, (N,)) * rng.uniform(0, 1.3, (N, 1))).T])
            out.append(dict(A=A, B=B, flags=fl, prm=(1.0, 1.0), kind="random", scale=s))
        for j, fl in enumerate(FLAGS):
            ma = np.concatenate([s * rng.standard_normal(3), CR._unit(rng, ()) * 0.9]); mb = np.concatenate([s * rng.standard_normal(3), CR._unit(rng, ()) * 0.7])
            A = _belief(rng, N, ma, 0.2 * s, 0.05); B = _belief(rng, N, mb, 0.1 * s, 0.02)
            out.append(dict(A=A, B=B, flags=fl, prm=((1.3, 0.8), (0.5, 2.0), (1.0, 1.0), (2.0, 1.0))[j], kind="belief", scale=s))
    return out


def anchor_cases(N):
    """a tight and a wide belief -> [(6, N)]"""
    rng = np.random.default_rng(2000 + N)
    return [_belief(rng, N, [3.0, -2.0, 1.0, 0.4, -0.8, 0.3], 0.01, 0.001), _belief(rng, N, [-30.0, 5.0, 12.0, -1.2, 0.5, 2.0], 2.0, 0.5)]


def mp_subset(N):
    """the particles the mp side serves: the first three and the last three (N = 257: the strided loop's second round)"""
    return sorted(set(range(min(N, 3))) | set(range(max(0, N - 3), N)))


@functools.lru_cache(maxsize=None)
def reference(N):
    """-> dict: cases, anchors, f64 outputs (compose `D`, final `out`, `anchor`), mp elements on mp_subset(N), per-case translation
    scale, zone mask per case (N,), dev and bound per block kind ("compose_t", "compose_r", "inflate_t", ...; relative to the scale)"""
    cs, an = cases(N), anchor_cases(N)
    idx = mp_subset(N)
    D = [compose3(c["A"], c["B"], *c["flags"]) for c in cs]
    out = [inflate3(d, *c["prm"]) for d, c in zip(D, cs)]
    anc = [anchor_mean3(a) for a in an]
    tscale = [max(1.0, float(np.abs(c["A"][:3]).max()), float(np.abs(c["B"][:3]).max()), float(np.abs(o[:3]).max())) for c, o in zip(cs, out)]
    ascale = [max(1.0, float(np.abs(a[:3]).max())) for a in an]
    dev = {k: 0.0 for k in ("compose_t", "compose_r", "inflate_t", "inflate_r", "anchor_t", "anchor_r")}
    zone, margin = [], math.inf
    mp_D, mp_out, mp_anchor = [], [], []
    with mpm.workdps(DPS):
        for c, d, o, ts in zip(cs, D, out, tscale):
            els = [mp_compose3(c["A"], c["B"], i, *c["flags"]) for i in idx]
            qw = np.array([float(e[1][0]) for e in els])
            th = np.array([float(mq_angle(e[1])) for e in els])
            inflated = c["prm"] != (1.0, 1.0)
            if inflated:
                el2 = mp_inflate3(d, idx, *c["prm"])
                th = np.concatenate([th, [float(mq_angle(e[1])) for e in el2]])
            margin = min(margin, float(np.abs((math.pi - th) - CR.ZONE_EDGE).min()))
            z = 2.0 * qw * qw <= SQRT_EPS
            zone.append(z)
            for r, i in enumerate(idx):
                et, er = mp_distance(d[:, i], els[r])
                dev["compose_t"] = max(dev["compose_t"], et / ts)
                if not z[r]:
                    dev["compose_r"] = max(dev["compose_r"], er)
                if inflated:
                    et, er = mp_distance(o[:, i], el2[r])
                    dev["inflate_t"] = max(dev["inflate_t"], et / ts); dev["inflate_r"] = max(dev["inflate_r"], er)
            mp_D.append(els); mp_out.append(el2 if inflated else els)
        for a, o, ts in zip(an, anc, ascale):
            el = mp_mean3(a)
            et, er = mp_distance(o[:, 0], el)
            dev["anchor_t"] = max(dev["anchor_t"], et / ts); dev["anchor_r"] = max(dev["anchor_r"], er)
            mp_anchor.append(el)
    # zone membership of EVERY particle, from the float64 quaternion of the composition (the margin above keeps it from tying)
    zone_all = []
    for c in cs:
        ta, qa = load3(c["A"]); tb, qb = load3(c["B"])
        if c["flags"][0]:
            ta, qa = invert3(ta, qa)
        if c["flags"][1]:
            tb, qb = invert3(tb, qb)
        zone_all.append(2.0 * q_mul(qa, qb)[:, 0] ** 2 <= SQRT_EPS)
    bound = {k: max(8.0 * v, 64.0 * EPS) for k, v in dev.items()}
    return dict(cases=cs, anchors=an, D=D, out=out, anchor=anc, idx=idx, mp_D=mp_D, mp_out=mp_out, mp_anchor=mp_anchor, tscale=tscale, ascale=ascale,
                zone=zone_all, zone_mp=zone, margin=margin, dev=dev, bound=bound)


def check_blocks(got, ref, what, inflated=True):
    """the device's (or any) outputs `got` [(6, N)] of the case table against reference(N) `ref`: float64 on every particle, mp on the subset,
    by the bound rule; the snap zone by its own rule (|ω| = π within 4 ulp, axis within the bound).  inflated=False: the plain compositions
    of every case (a plan without params).  -> figures (units of the bound)"""
    fig = {"t64": 0.0, "r64": 0.0, "tmp": 0.0, "rmp": 0.0}
    mp_ref = ref["mp_out"] if inflated else ref["mp_D"]
    for j, (c, g, o, ts, z) in enumerate(zip(ref["cases"], got, ref["out"] if inflated else ref["D"], ref["tscale"], ref["zone"])):
        k = "inflate" if inflated and c["prm"] != (1.0, 1.0) else "compose"
        bt, br = ref["bound"][k + "_t"] * ts, ref["bound"][k + "_r"]
        assert np.isfinite(g).all(), (what, j)
        et, er = np_distance(g, o)
        fig["t64"] = max(fig["t64"], float((et / bt).max())); fig["r64"] = max(fig["r64"], float(np.where(z, 0.0, er / br).max()))
        assert (et <= bt).all(), (what, j, c["kind"], c["flags"], float((et / bt).max()))
        assert ((er <= br) | z).all(), (what, j, c["kind"], c["flags"], float(np.where(z, 0.0, er / br).max()))
        if z.any():
            w = g[3:, z].T
            nw = np.sqrt((w * w).sum(-1))
            assert (np.abs(nw - math.pi) <= 4 * CR.ULP_PI).all(), (what, j, "snap zone: |ω| is not π")
            wo = o[3:, z].T
            ax = wo / np.sqrt((wo * wo).sum(-1))[:, None]
            da = np.minimum(np.abs(w / nw[:, None] - ax).max(-1), np.abs(w / nw[:, None] + ax).max(-1))
            assert (da <= br).all(), (what, j, "snap zone: axis")
        with mpm.workdps(DPS):
            for r, i in enumerate(ref["idx"]):
                e_t, e_r = mp_distance(g[:, i], mp_ref[j][r])
                fig["tmp"] = max(fig["tmp"], e_t / bt)
                assert e_t <= bt, (what, j, i, e_t / bt)
                if not z[i]:
                    fig["rmp"] = max(fig["rmp"], e_r / br)
                    assert e_r <= br, (what, j, i, e_r / br)
    return fig


def check_anchors(got, ref, what):
    fig = {"t": 0.0, "r": 0.0}
    for j, (g, o, el, ts) in enumerate(zip(got, ref["anchor"], ref["mp_anchor"], ref["ascale"])):
        bt, br = ref["bound"]["anchor_t"] * ts, ref["bound"]["anchor_r"]
        assert np.isfinite(g).all() and (g == g[:, :1]).all(), (what, j)          # N copies of one point
        et, er = np_distance(g, o)
        with mpm.workdps(DPS):
            mt, mr = mp_distance(g[:, 0], el)
        fig["t"] = max(fig["t"], float(et.max() / bt), mt / bt); fig["r"] = max(fig["r"], float(er.max() / br), mr / br)
        assert et.max() <= bt and er.max() <= br and mt <= bt and mr <= br, (what, j, fig)
    return fig


# ------------------------------------------------------------------------------------------------------------ the solver's oracle backend
class Elim3BlockOp(OracleTreeBlockOp):
    """OracleTreeBlockOp + "compose" on Pose3 blocks + "anchor_mean" (Pose3: the mean point; Pose2 / Point2: "anchor")"""

    def run(self):
        v = self.store.vals
        if self.op == "anchor_mean":
            for e in self.entries:
                if v[e[0]].shape[0] == 6:
                    v[e[1]] = anchor_mean3(v[e[0]])
                else:
                    OracleTreeBlockOp(self.store, "anchor", [e]).run()
        elif self.op == "compose" and self.entries and v[self.entries[0][0]].shape[0] == 6:
            for e in self.entries:
                D = compose3(v[e[0]], v[e[1]], bool(e[3]), bool(e[4]))
                v[e[2]] = inflate3(D, float(e[5]), float(e[6])) if len(e) > 5 else D
        else:
            super().run()


def upsolve_ref3(R, L, order, N, seed, gibbs_iters, groups, stream_offset, stream_ids, up_stream, solver, messages, meas_vals, pairs):
    """tests/solve_ref.py upsolve_ref for a level of Pose3 variables, the p3p3 family only: ordinary, prior (direction 2) and SAMPLED rows --
    the latter through conv_pose3pose3(noise = the samples' block) on the row's <sampled> factor entry (mu = 0, cov = I: z = the samples).
    Same rows, Philox streams (5 << 28 rows, 6 << 28 products), bandwidth rule and product as the device's plan."""
    import oracle as ro
    from rome_jl_amd.clique import CliqueBatch
    batch = CliqueBatch(L, pairs)
    for l in order:
        if l not in batch.vidx:
            batch.vidx[l] = len(batch.vars[R.Pose3]); batch.vars[R.Pose3].append(l)
    assert not any(batch.fam_rows[f] for f in ("p2p2", "br1", "br0", "prpt2"))
    bel = batch.beliefs(R.Pose3)
    rows = np.array(batch.fam_rows["p3p3"], dtype=np.int64).reshape(-1, 4)
    T = batch.tabs["p3p3"]
    mu3 = np.array(T["mu"]).reshape(-1, 6)
    L3 = np.array([ro.cholesky_lower(np.asarray(c).reshape(6, 6)) for c in T["spread"]]).reshape(-1, 21)
    sid = list(range(len(rows)))
    flabel = [None] * len(rows)
    for pair, (fam, r) in batch.rows.items():
        sid[r] = stream_ids[pair]; flabel[r] = pair[0]
    for it in range(gibbs_iters):
        base = stream_offset + (it << 32)
        for gg in sorted(set(groups)):
            group = [l for l, g in zip(order, groups) if g == gg]
            tv = {batch.vidx[l]: l for l in group}
            props = {l: [] for l in group}
            for r in range(len(rows)):
                f, d, fx, tg = rows[r]
                if tg not in tv:
                    continue
                so = base + (5 << 28) + sid[r]
                if d == 2:
                    p = ro.sample_priorpose3(ro.make_opts(N=N, seed=seed, stream_offset=so), mu3[f], L3[f])[0]
                else:
                    nz = None
                    if batch.fam_meas["p3p3"][r] != -1:
                        nz = np.asarray(meas_vals[L.getFactor(flabel[r])[2].meas], dtype=float)[None]
                    o = ro.make_opts(N=N, solver=solver, seed=seed, stream_offset=so, nullhypo=batch.fam_hyp["p3p3"][r][2])
                    p = ro.conv_pose3pose3(o, mu3, L3, bel, [fx], [tg], [d], factor=[f], noise=nz)[0]
                props[tv[tg]].append(p)
            for l in group:
                for pts in (messages or {}).get(l, []):
                    props[l].append(np.asarray(pts, dtype=float))
            ls = [l for l in group if props[l]]
            if not ls:
                continue
            P = np.concatenate([np.stack(props[l]) for l in ls])
            ptr = np.concatenate([[0], np.cumsum([len(props[l]) for l in ls])]).astype(np.int32)
            bw = ro.kde_bandwidths(P, 0b111000)
            new = {}
            for k, l in enumerate(ls):
                o = ro.make_opts(N=N, seed=seed, stream_offset=base + (6 << 28) + up_stream[l])
                Pk, bk = P[ptr[k]:ptr[k + 1]], bw[ptr[k]:ptr[k + 1]]
                new[l] = ro.product_msgibbs(o, 6, np.array([0, len(Pk)], dtype=np.int32), np.arange(len(Pk), dtype=np.int32), Pk, bk,
                                            bel[batch.vidx[l]][None], 0, 1)[0]
            for l, b in new.items():
                bel[batch.vidx[l]] = b
    return {l: bel[batch.vidx[l]].copy() for l in order}


class Elim3Plan(OracleTreePlan):
    def run(self, opts, mirror_out=None, mirror_stride=0):
        st, sp = self.store, self.spec
        L = sp.fg
        if any(vt is not st.R.Pose3 for vt in L.variables.values()) or self.share is not None or self.mirror is not None:
            return super().run(opts, mirror_out, mirror_stride)
        L.vals = {l: st.vals[l] for l in L.variables if l in st.vals}
        msgs = {}
        for src, dst in sp.smsgs:
            msgs.setdefault(dst, []).append(st.vals[src])
        ref = upsolve_ref3(st.R, L, list(sp.order), st.N, int(opts.seed), sp.gibbs_iters, list(sp.groups), int(opts.stream_offset), self.sid,
                           self.pos_t, int(opts.solver), msgs, st.vals, list(sp.pairs))
        for l in sp.order:
            st.vals[l] = ref[l]


class Elim3Backend(OracleTreeBackend):
    def Plan(self, store, spec, share=None, mirror=None):
        return Elim3Plan(store, spec, share=share, mirror=mirror)

    def BlockOp(self, store, op, entries):
        return Elim3BlockOp(store, op, entries)
