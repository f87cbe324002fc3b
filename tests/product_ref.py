"""References for the importance product (k_product<M,S>: Flat<2>, Flat<3>, Se3M) and the belief statistics (k_belief_stats<D>, block_stats) of
rome.jl_amd/csrc/rome_product.hip: what rome_product_dev / rome_product_bw_dev / rome_belief_stats* must return for every particle.

Three sides, none of which is the kernel:
  * mp_spread / mp_product -- mpmath at lin_ref.DPS digits on GROUP ELEMENTS (headings through _wrap, rotation matrices through
                              lin_ref's _so3_exp / _so3_log), one belief block / one variable.
  * np_spread / np_product -- float64 NumPy over a whole table, written the plain way and NOT in the kernel's order: two-pass moments,
                              max-shifted log-sum-exp over all N kernel points at once, np.cumsum, np.searchsorted(c, τ, "right")
                              clipped to N − 1, SE(3) differences through unit quaternions (conv_ref's q_* helpers).
  * the C oracle (ro.product, ro.belief_spread), in tests/test_product_ref_host.py only: same author, same operation order as the
    kernel, so it is not the independent side; it ties the row scatter, the Philox streams and the floor of np_product to it.

Definition restated (the comment above ro_product_bw in oracle/rome_oracle.c).  Proposal l of a variable (row prop_rows[ptr[v] + l] of
`prop`): bandwidth h_lk = max(c_N·sd_lk, 1e-6), c_N = (4/((D+2)N))^(1/(D+4)), sd about particle 0 -- or max(prop_bw[row, k], 1e-6) when
bandwidths are supplied.  Base = the proposal with the smallest Σ_k log h_lk, ties to the lowest l.  log w_i = Σ_{l≠base} log Σ_j
exp(−½ Σ_k (d(x_i, y_lj)_k / h_lk)²) over the N base points x_i.  One uniform u = (w₀ + ½)/2³² from Philox counter (0xFFFFFFFF, stream,
3 << 16), stream = stream_offset + v; output particle i picks the first m with c_m > (i + u)/N (c: normalised cumulative weights), else
N − 1, and is x_m ⊕ h_p⊙ξ_i with 1/h_p,k² = Σ_l 1/h_lk² and ξ_i = ro.rng_normals(seed, stream_offset + v, i, D).  K = 1 copies the
proposal, K = 0 keeps the belief.

Comparison rule -- every particle decided, none left out.  Picks are discrete, so the reference alone evaluates a margin: for output
particle i, g_i = min_m |(i + u)/N − c_m| over the distinct values of its c.  δ = max(8·dev_c, 64 ulp) x scale is the bound on a correct
double evaluation of c in another order, where scale = max(1, largest |log-weight term −½q_min + log Σ| of the table) (far-apart
proposals carry their rounding in −½·q_min) and dev_c = largest |c_np − c_mp| on the mp variables of the table kind, relative to the
variable's own scale (as conv_ref's dev is relative to the row scale).  CONDITIONS, checked on the CPU (test_product_ref_host.py): every
table has min_i g_i >= 1000·δ, and the two smallest Σ log h of every variable are bit-equal by construction or >= 1000·(64 ulp·D)
apart.  A table that misses one of the two, or (D = 6) the 1e-5 clearance of the snap zone's edge named below, gets another seed
(RESEED).  On the GPU no particle is excluded:
  * the pick of every particle, recovered from out ⊖ h_p⊙ξ as the nearest base particle (which must lie within the output bound), equals
    the reference's;
  * out = Pb[pick] ⊕ h_p⊙ξ within max(8·dev_out, 64 ulp) x max(1, largest |coordinate| of the variable's proposals), translation part
    and rotation part separately (wrapped heading / angle of Refᵀ·Exp(ω)), with conv_ref's snap-zone rule for D = 6 outputs within
    acos(1 − √eps) of π (membership from the reference's own q_w; every table keeps 1e-5 clear of the zone's edge);
  * K = 0 and K = 1 blocks are bit-equal to their source.
Belief statistics: sd within max(8·dev, 64 ulp) x max(1, largest |tangent difference| of the block); mean, as a group element, within
the same factor x max(1, largest |tangent difference|, largest |coordinate|).  The Pose2 mean heading is θ₀ + mean d, not reduced to
(−π, π] (the oracle's definition too), hence compared wrapped.

Measured dev (CPU, np against mp, printed by tests/test_product_ref_host.py -s), in units of eps = 2^-52:
  dev_c     shape <= 0.69   large-K <= 4.02 (N = 16, K = 33: 32 terms per weight)   tie / floor <= 0.06   far-apart 0.00
  dev_out   translation <= 0.47   rotation <= 0.03      (all kinds, D = 2 / 3 / 6)
  dev_stats mean <= 0.42 translation, <= 0.02 rotation    sd <= 1.17
Every 8·dev lies below the floor, so every bound is the floor, 64 ulp = 1.42e-14 times its scale.  The host test holds every dev under
8 eps, so a table cannot move a bound without failing there first.  About 70 000 output particles are decided in all, none excluded.
"""
import functools
import math

import mpmath as mpm
import numpy as np

import conv_ref as CR
from conv_ref import q_conj, q_exp, q_log, q_mul
from lin_ref import DPS, EPS, SQRT_EPS, _mm, _mt, _so3_exp, _so3_log, _wrap

FLOOR = 1e-6
ULP64 = 64.0 * EPS
SEED = 0x50524F44
DIMS = (2, 3, 6)
NT = {2: 2, 3: 2, 6: 3}                                    # translation coordinates
KIND = {2: CR.BR0, 3: CR.P2P2, 6: CR.P3P3}                  # conv_ref's element kinds: (t,), (t, θ), (t, R)
SILVERMAN, SUPPLIED = "silverman", "bw"
MODES = (SILVERMAN, SUPPLIED)
GAP_FACTOR = 1000.0

# ------------------------------------------------------------------------------------------------------------ launch arithmetic
PROD_WAVES, PROD_CHUNK, PROD_MAXK, PROD_MAXN, PROD_MAXN_SE3 = 4, 8, 32, 512, 256   # kProdWaves, kProdChunk, kProdMaxK, kProdMaxN, SE(3)


def launch_shape(D, N, K):
    """what launch_product instantiates for one variable: slots per lane S, block-phase particles per thread T4, idle slots of the last
    64-group, LDS trips over the non-base proposals, their sizes, and whether the bandwidths stay cached"""
    S = 1 if N <= 64 else 2 if N <= 128 else 4 if N <= 256 else 8
    trips = -(-(K - 1) // PROD_CHUNK) if K > 1 else 0
    return {"S": S, "T4": -(-S // PROD_WAVES), "idle": 64 * S - N, "trips": trips,
            "chunks": [min(PROD_CHUNK, K - 1 - c0) for c0 in range(0, max(K - 1, 0), PROD_CHUNK)],
            "cached": K <= PROD_MAXK, "bw_chunks": -(-K // PROD_MAXK), "staged": D == 6 or S <= 4}


SHAPE_N = {2: (1, 2, 63, 64, 65, 128, 129, 256, 257, 512), 3: (1, 2, 63, 64, 65, 128, 129, 256, 257, 512),
           6: (1, 2, 63, 64, 65, 128, 129, 256)}
SHAPE_K = (0, 1, 2, 3, 4, 5, 6, 9, 10, 17, 18)              # wave dealing of 1..5 proposals, chunk edges 8 | 9 and 16 | 17
LARGE_N, LARGE_K = (16, 65), (32, 33, 34, 65)
MP_SHAPE_N, MP_SHAPE_K = 65, 3                               # the mp variable of the shape tables
# table key -> seed bump, for a table whose fixed seed missed a CPU condition.  All five missed only the 1e-5 clearance of the snap
# zone's edge (margins 2.3e-6 .. 7.8e-6 at bump 0): the edge variables put many outputs near π.  None missed the pick gap or Σ log h.
RESEED = {
    ("shape", 6, 63, "bw"): 1,
    ("shape", 6, 65, "bw"): 1,
    ("shape", 6, 128, "bw"): 1,
    ("shape", 6, 129, "bw"): 2,
    ("shape", 6, 256, "bw"): 2,
}


# ------------------------------------------------------------------------------------------------------------ float64 side
def _remainder(x):
    """x − 2π·round(x / 2π) with 2π in two parts (|x| stays below a few turns here)"""
    x = np.asarray(x, dtype=np.float64)
    k = np.rint(x / (2.0 * math.pi))
    return (x - k * 6.283185307179586) - k * 2.4492935982947064e-16


def tangent_about(D, X, Y):
    """d(x, y) of the definition, broadcasting over leading axes; X, Y (..., D): (x.t − y.t, wrap(θx − θy) | Log(R_yᵀ R_x))"""
    d = np.array(np.broadcast_arrays(X - Y)[0])
    if D == 3:
        d[..., 2] = _remainder(d[..., 2])
    elif D == 6:
        d[..., 3:] = q_log(q_mul(q_conj(q_exp(Y[..., 3:])), q_exp(X[..., 3:])))
    return d


def np_spread(blk):
    """blk (D, N) -> dict: d (N, D) tangent coordinates about particle 0, md their mean, sd (n − 1; N = 1: 0), and the mean as a group
    element: t, and th (θ₀ + mean d, unreduced) | q"""
    blk = np.asarray(blk, dtype=np.float64)
    D, N = blk.shape
    X = blk.T
    d = tangent_about(D, X, X[:1])
    md = d.mean(axis=0)
    e = d - md
    sd = np.sqrt((e * e).sum(axis=0) / max(N - 1, 1))
    out = {"d": d, "md": md, "sd": sd, "t": X[0, :NT[D]] + md[:NT[D]]}
    if D == 3:
        out["th"] = X[0, 2] + md[2]
    if D == 6:
        out["q"] = q_mul(q_exp(X[0, 3:]), q_exp(md[3:]))
    return out


def silverman_factor(D, N):
    return (4.0 / ((D + 2.0) * N)) ** (1.0 / (D + 4.0))


def uniform3(seed, stream):
    """the resampling uniform: Philox domain 3 on `stream`"""
    import oracle as ro
    w = ro.philox([0xFFFFFFFF, stream & 0xFFFFFFFF, stream >> 32, 3 << 16], [seed & 0xFFFFFFFF, seed >> 32])
    return (w[0] + 0.5) / 4294967296.0


def _lse_terms(D, X, Y, h):
    """log Σ_j exp(−½ q_ij), q_ij = Σ_k (d(x_i, y_j)_k / h_k)², max-shifted over j -> (N,)"""
    d = tangent_about(D, X[:, None, :], Y[None, :, :]) / h
    e = -0.5 * (d * d).sum(axis=-1)
    mx = e.max(axis=1)
    return mx + np.log(np.exp(e - mx[:, None]).sum(axis=1))


def bandwidths(t, v):
    """(K, D) floored bandwidths of the proposals of variable v"""
    D, N = t["D"], t["N"]
    rows = t["rows"][t["ptr"][v]:t["ptr"][v + 1]]
    if t["bw"] is not None:
        raw = t["bw"][rows]
    else:
        raw = silverman_factor(D, N) * np.array([np_spread(t["prop"][r])["sd"] for r in rows]).reshape(len(rows), D)
    return np.maximum(raw, FLOOR)


def jitter(D, x, e):
    """x ⊕ e on coordinates x (N, D) -> element dict t, th | q (heading unreduced: compared wrapped)"""
    out = {"t": x[:, :NT[D]] + e[:, :NT[D]]}
    if D == 3:
        out["th"] = x[:, 2] + e[:, 2]
    if D == 6:
        out["q"] = q_mul(q_exp(x[:, 3:]), q_exp(e[:, 3:]))
    return out


def np_product(t, xi=None):
    """per variable with K >= 2: base, h (K, D), lnh (K,), hp (D,), terms (K − 1, N), logw, c, u, picks, out (element dict over N);
    K < 2: {"K": K, "src": the block to copy}"""
    D, N, ptr, rows = t["D"], t["N"], t["ptr"], t["rows"]
    V = len(ptr) - 1
    if xi is None:
        xi = CR.normals(t["seed"], t["stream_offset"], V, N, D)
    res = []
    for v in range(V):
        rv = rows[ptr[v]:ptr[v + 1]]
        K = len(rv)
        if K < 2:
            res.append({"K": K, "src": t["bel"][v] if K == 0 else t["prop"][rv[0]]})
            continue
        h = bandwidths(t, v)
        lnh = np.log(h).sum(axis=1)
        base = int(np.argmin(lnh))                                              # the first of equal minima
        X = t["prop"][rv[base]].T
        with np.errstate(all="ignore"):
            terms = np.array([_lse_terms(D, X, t["prop"][rv[l]].T, h[l]) for l in range(K) if l != base])
        logw = terms.sum(axis=0)
        w = np.exp(logw - logw.max())
        cum = np.cumsum(w)
        c = cum / cum[-1]
        u = uniform3(t["seed"], t["stream_offset"] + v)
        tau = (np.arange(N) + u) / N
        picks = np.minimum(np.searchsorted(c, tau, side="right"), N - 1)
        hp = 1.0 / np.sqrt((1.0 / (h * h)).sum(axis=0))
        res.append({"K": K, "base": base, "h": h, "lnh": lnh, "hp": hp, "terms": terms, "logw": logw, "c": c, "u": u, "tau": tau,
                    "picks": picks, "out": jitter(D, X[picks], hp * xi[v]), "scale_w": max(1.0, float(np.abs(terms).max())),
                    "scale_x": max(1.0, float(np.abs(t["prop"][rv]).max()))})
    return res


def pick_gap(r):
    """min_i g_i of one variable: the distance of every τ_i to the nearest distinct cumulative weight.  c_{N−1} = 1 is left out: a
    search that runs past the end is clipped to N − 1, so the last cumulative weight decides no pick (N = 1: no boundary at all)."""
    cv = np.unique(r["c"][:-1])
    if len(cv) == 0:
        return math.inf
    j = np.clip(np.searchsorted(cv, r["tau"]), 1, len(cv) - 1) if len(cv) > 1 else np.zeros(len(r["tau"]), int)
    lo = np.abs(r["tau"] - cv[np.maximum(j - 1, 0)])
    return float(np.minimum(lo, np.abs(r["tau"] - cv[j])).min())


def lnh_gap(r):
    """(gap between the two smallest Σ log h, whether they are bit-equal)"""
    s = np.sort(r["lnh"])
    return float(s[1] - s[0]), bool(s[1] == s[0])


def coords_to_elements(D, blk):
    """SoA block (D, N) -> element dict over N"""
    X = np.asarray(blk).T
    out = {"t": X[:, :NT[D]]}
    if D == 3:
        out["th"] = X[:, 2]
    if D == 6:
        out["q"] = q_exp(X[:, 3:])
    return out


def element_distance(D, a, b):
    """(translation error, rotation error) between element dicts, broadcasting"""
    et = np.abs(a["t"] - b["t"]).max(axis=-1)
    if D == 2:
        return et, np.zeros_like(et)
    if D == 3:
        return et, np.abs(_remainder(a["th"] - b["th"]))
    return et, CR.q_angle(q_mul(q_conj(b["q"]), a["q"]))


def zone_of(q):
    """snap-zone membership of reference quaternions and the angle to π (accurate near π), as conv_ref.Reference does"""
    qw2 = 2.0 * q[..., 0] ** 2 / np.sum(q * q, axis=-1)
    return qw2 <= SQRT_EPS, 2.0 * np.arctan2(np.abs(q[..., 0]), np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1)))


# ------------------------------------------------------------------------------------------------------------ mpmath side
def _f(v):
    return mpm.mpf(float(v))


def _mp_elem(D, x):
    x = [_f(v) for v in x]
    if D == 2:
        return (x,)
    if D == 3:
        return (x[:2], x[2])
    return (x[:3], _so3_exp(x[3:]))


def _mp_diff(D, a, b):
    """d(a, b) on mp elements"""
    d = [x - y for x, y in zip(a[0], b[0])]
    if D == 3:
        d.append(_wrap(a[1] - b[1]))
    if D == 6:
        d += _so3_log(_mm(_mt(b[1]), a[1]))
    return d


def mp_spread(blk):
    """one block (D, N) at the current mp precision -> (mean element, sd list, largest |d|)"""
    blk = np.asarray(blk, dtype=np.float64)
    D, N = blk.shape
    els = [_mp_elem(D, blk[:, i]) for i in range(N)]
    d = [_mp_diff(D, e, els[0]) for e in els]
    md = [sum(di[k] for di in d) / N for k in range(D)]
    sd = [mpm.sqrt(sum((di[k] - md[k]) ** 2 for di in d) / max(N - 1, 1)) for k in range(D)]
    t = [els[0][0][k] + md[k] for k in range(NT[D])]
    if D == 2:
        mean = (t,)
    elif D == 3:
        mean = (t, els[0][1] + md[2])
    else:
        mean = (t, _mm(els[0][1], _so3_exp(md[3:])))
    return mean, sd, max(abs(x) for di in d for x in di)


def mp_product(t, v, xi_v):
    """one variable (K >= 2) at the current mp precision -> base, h, hp, logw, c, picks, out (list of mp elements)"""
    D, N = t["D"], t["N"]
    rv = t["rows"][t["ptr"][v]:t["ptr"][v + 1]]
    K = len(rv)
    if t["bw"] is not None:
        raw = [[_f(x) for x in t["bw"][r]] for r in rv]
    else:
        cn = (mpm.mpf(4) / ((D + 2) * N)) ** (mpm.mpf(1) / (D + 4))
        raw = [[cn * s for s in mp_spread(t["prop"][r])[1]] for r in rv]
    h = [[max(x, _f(FLOOR)) for x in row] for row in raw]
    lnh = [sum(mpm.log(x) for x in row) for row in h]
    base = min(range(K), key=lambda l: (lnh[l], l))
    els = [[_mp_elem(D, t["prop"][r][:, j]) for j in range(N)] for r in rv]
    logw = []
    for i in range(N):
        acc = mpm.mpf(0)
        for l in range(K):
            if l == base:
                continue
            s = mpm.mpf(0)
            for j in range(N):
                d = _mp_diff(D, els[base][i], els[l][j])
                s += mpm.exp(-sum((d[k] / h[l][k]) ** 2 for k in range(D)) / 2)
            acc += mpm.log(s)
        logw.append(acc)
    mx = max(logw)
    w = [mpm.exp(x - mx) for x in logw]
    tot = sum(w)
    c, run = [], mpm.mpf(0)
    for x in w:
        run += x
        c.append(run / tot)
    u = _f(uniform3(t["seed"], t["stream_offset"] + v))                         # u is a double by definition
    picks = []
    for i in range(N):
        tau = (i + u) / N
        picks.append(next((m for m in range(N) if c[m] > tau), N - 1))
    hp = [1 / mpm.sqrt(sum(1 / (h[l][k] * h[l][k]) for l in range(K))) for k in range(D)]
    out = []
    for i in range(N):
        p = els[base][picks[i]]
        e = [hp[k] * _f(xi_v[i, k]) for k in range(D)]
        tt = [p[0][k] + e[k] for k in range(NT[D])]
        out.append((tt,) if D == 2 else (tt, p[1] + e[2]) if D == 3 else (tt, _mm(p[1], _so3_exp(e[3:]))))
    return {"base": base, "h": h, "hp": hp, "logw": logw, "c": c, "picks": picks, "out": out}


def _np_as_mp_element(D, el, i):
    tt = [_f(x) for x in el["t"][i]]
    return (tt,) if D == 2 else (tt, _f(el["th"][i])) if D == 3 else (tt, CR._mp_quat_matrix(el["q"][i]))


# ------------------------------------------------------------------------------------------------------------ proposal tables
def _unit(rng, shape=()):
    v = rng.standard_normal(shape + (3,))
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def _centre(rng, D, edge):
    """centre coordinates of a variable; edge: heading at ±π (D = 3), |ω| within 1e-3 of π (D = 6)"""
    c = np.zeros(D)
    c[:NT[D]] = rng.uniform(-100, 100, NT[D])
    if D == 3:
        c[2] = math.pi - 0.05 * rng.uniform(0, 1) if edge else rng.uniform(-2.5, 2.5)
    if D == 6:
        c[3:] = _unit(rng) * (math.pi - 1e-3 * rng.uniform(0.6, 1.0) if edge else rng.uniform(0, 2.0))
    return c


def _compose(D, c, e):
    """c ⊕ e as coordinates (N, D): headings wrapped to (−π, π], rotation vectors principal"""
    x = c[None, :] + e
    if D == 3:
        x[:, 2] = np.arctan2(np.sin(x[:, 2]), np.cos(x[:, 2]))
    if D == 6:
        x[:, 3:] = q_log(q_mul(q_exp(np.broadcast_to(c[3:], e[:, 3:].shape)), q_exp(e[:, 3:])))
    return x


SIG0 = {2: np.array([1.0, 1.0]), 3: np.array([1.0, 1.0, 0.15]), 6: np.array([1.0, 1.0, 1.0, 0.1, 0.1, 0.1])}


def _proposal(rng, D, N, c, scale, bimodal, edge):
    """one proposal block (D, N) about c and the per-coordinate sigma it was drawn with"""
    sig = SIG0[D] * scale * rng.uniform(0.7, 1.5, D)
    e = 0.5 * sig * rng.standard_normal(D) + sig * rng.standard_normal((N, D))
    if bimodal:
        e[::2, 0] += 4.0 * sig[0]
    if D == 6 and edge and N >= 2:                                               # |ω| on both sides of the cut, 5e-4 from π
        ax = c[3:] / np.sqrt(np.sum(c[3:] ** 2))
        ang = math.sqrt(float(np.sum(c[3:] ** 2)))
        e[0, 3:] = ax * (math.pi - 5e-4 - ang)
        e[1, 3:] = ax * (math.pi + 5e-4 - ang)
    return _compose(D, c, e).T.copy(), sig


def _assemble(D, N, blocks, sigs, seed, stream_offset, mode, rng, n_unused=3, bw=None):
    """blocks: per variable a list of (D, N) proposals.  Rows are scattered over `prop` by a random permutation among unused rows."""
    V = len(blocks)
    Ks = [len(b) for b in blocks]
    R = sum(Ks) + n_unused
    perm = rng.permutation(R).astype(np.int32)
    prop = rng.standard_normal((R, D, N)) * 3.0                                   # unused rows hold ordinary finite data
    rows = perm[:sum(Ks)].copy()
    flat = [b for bl in blocks for b in bl]
    for r, b in zip(rows, flat):
        prop[r] = b
    t = {"D": D, "N": N, "ptr": np.concatenate([[0], np.cumsum(Ks)]).astype(np.int32), "rows": rows, "prop": prop,
         "bel": rng.standard_normal((V, D, N)) * 2.0, "seed": seed, "stream_offset": stream_offset, "mode": mode, "bw": None}
    if mode == SUPPLIED:
        if bw is None:
            if N > 2:                                                            # the lcv rule of the solve loop
                import oracle as ro
                full = ro.kde_bandwidths(prop, 0b100 if D == 3 else (0b111000 if D == 6 else 0))
            else:
                full = np.abs(rng.standard_normal((R, D))) + 0.1
                for r, s in zip(rows, [s for sl in sigs for s in sl]):
                    full[r] = 0.5 * s
        else:
            full = np.abs(rng.standard_normal((R, D))) + 0.1
            for r, b in zip(rows, [b for bl in bw for b in bl]):
                full[r] = b
        t["bw"] = np.ascontiguousarray(full)
    return t


def _variable(rng, D, N, K, base_at, edge, bimodal_every=3, base_scale=0.2, scale=1.0):
    c = _centre(rng, D, edge)
    out = [_proposal(rng, D, N, c, scale * (base_scale if l == base_at else 1.0), bimodal=(l % bimodal_every == 1), edge=edge) for l in range(K)]
    return [b for b, _ in out], [s for _, s in out]


def base_position(K, which):
    return {"first": 0, "middle": K // 2, "last": K - 1}[which] if K >= 2 else None


def _seed(key):
    D, N = key[1], key[2]
    return 7000 + 131 * DIMS.index(D) + 17 * N + 1009 * RESEED.get(key, 0) + {"shape": 0, "large": 1, "tie": 2, "far": 3}[key[0]] * 100003


@functools.lru_cache(maxsize=None)
def shape_table(D, N, mode):
    """V = 11 variables with K of SHAPE_K; the intended base goes first / middle / last in turn; every other variable is an edge variable
    (heading cluster across ±π, |ω| within 1e-3 of π); every third proposal is bimodal"""
    key = ("shape", D, N, mode)
    rng = np.random.default_rng(_seed(key))
    blocks, sigs, want = [], [], []
    for v, K in enumerate(SHAPE_K):
        pos = base_position(K, ("first", "middle", "last")[v % 3])
        b, s = _variable(rng, D, N, K, pos, edge=(v % 2 == 0))
        blocks.append(b); sigs.append(s); want.append(pos)
    t = _assemble(D, N, blocks, sigs, SEED + N, (1 << 32) + 777 if N == 65 else 500 + N, mode, rng)
    t["key"], t["want_base"] = key, want
    t["mp_vars"] = [SHAPE_K.index(MP_SHAPE_K)] if N == MP_SHAPE_N else []
    return t


LARGE_BASE = {32: 31, 33: 32, 34: 0, 65: 64}                                      # l = 31, 32, 0 and K − 1


@functools.lru_cache(maxsize=None)
def large_table(D, N, mode):
    """K in {32, 33, 34, 65}: the bandwidth cache at its limit and switched off; the base at l = 31, 32, 0 and K − 1, then each K once
    more with the base moved (l = 0, 31, 32, 31)"""
    key = ("large", D, N, mode)
    rng = np.random.default_rng(_seed(key))
    blocks, sigs, want = [], [], []
    for K, pos in list(LARGE_BASE.items()) + [(32, 0), (33, 31), (34, 32), (65, 31)]:
        b, s = _variable(rng, D, N, K, pos, edge=(K % 2 == 0), bimodal_every=5)
        blocks.append(b); sigs.append(s); want.append(pos)
    t = _assemble(D, N, blocks, sigs, SEED + 1000 + N, 9000 + N, mode, rng)
    t["key"], t["want_base"] = key, want
    t["mp_vars"] = [1] if N == 16 else []                                         # K = 33, base in the second 32-chunk
    return t


TIE_K40 = 40


@functools.lru_cache(maxsize=None)
def tie_table(D, N=24):
    """supplied bandwidths: bit-identical bandwidth rows on different points (the lowest l must become the base), one pair with a member
    in each 32-chunk of a K = 40 variable, and entries of 0, 1e-9 and 1e-6 (all floored to 1e-6)"""
    key = ("tie", D, N, SUPPLIED)
    rng = np.random.default_rng(_seed(key))
    blocks, sigs, bws, want = [], [], [], []

    tiny = np.where(np.arange(D) < NT[D], 2e-6, 1.0)                             # translations within a few floors of one another

    def var(K, tied, row, floor_rows=()):
        b, s = _variable(rng, D, N, K, None, edge=False, base_scale=1.0, scale=tiny if floor_rows else 1.0, bimodal_every=10 ** 6 if floor_rows else 3)
        bw = [x * (5.0 if floor_rows else 0.5) for x in s]
        for l in tied:
            bw[l] = np.array(row, dtype=np.float64)
        for l, val in floor_rows:                                                 # translation entries at / below the floor, one shared rotation row
            bw[l] = np.where(np.arange(D) < NT[D], val, 0.5 * SIG0[D])
        blocks.append(b); sigs.append(s); bws.append(bw); want.append(min(tied) if tied else None)
    tight = 0.05 * SIG0[D]
    var(3, (1, 2), tight)                                                         # tie in the middle and last: l = 1
    var(4, (0, 3), tight)                                                         # first and last: l = 0
    var(5, (2, 3, 4), tight)                                                      # three-way
    var(TIE_K40, (7, 35), tight)                                                  # one member per 32-chunk: l = 7
    var(TIE_K40, (31, 32), tight)                                                 # across the chunk edge: l = 31
    # the floor: 0, 1e-9 and 1e-6 all become 1e-6 -- three proposals tie at D·log(1e-6), l = 1 is the base
    var(4, (), None, floor_rows=((1, 0.0), (2, 1e-9), (3, 1e-6)))
    want[-1] = 1
    # one floored coordinate only (no tie): the floor enters h and hp
    b, s = _variable(rng, D, N, 3, None, edge=False, base_scale=1.0)
    bw = [0.5 * x for x in s]; bw[2] = bw[2].copy(); bw[2][0] = 1e-9
    blocks.append(b); sigs.append(s); bws.append(bw); want.append(2)
    t = _assemble(D, N, blocks, sigs, SEED + 2000, 12000, SUPPLIED, rng, bw=bws)
    t["key"], t["want_base"], t["mp_vars"] = key, want, [0, 5]
    t["tied"] = [(1, 2), (0, 3), (2, 3, 4), (7, 35), (31, 32), (1, 2, 3), ()]
    return t


def _dyadic(rng, shape, scale):
    """multiples of 2^-10: sums and differences of a few of them are exact in double"""
    return np.round(rng.uniform(-scale, scale, shape) * 1024.0) / 1024.0


@functools.lru_cache(maxsize=None)
def small_n_table(D, N):
    """N = 1 and N = 2 under Silverman's rule.  N = 1: every sd is 0, every h the floor, every Σ log h equal -> base l = 0.  N = 2: the
    two points of every proposal of a variable differ by the SAME dyadic offset (translations; one shared pair of
    headings / rotations), so every sd -- a function of that offset alone -- is bit-equal in any arithmetic, and so is every h."""
    key = ("tie", D, N, SILVERMAN)
    rng = np.random.default_rng(_seed(key))
    blocks = []
    for K in (2, 3, 5, 9, 0, 1):
        c = _dyadic(rng, D, 50.0)
        if D >= 3:
            c[NT[D]:] = _dyadic(rng, D - NT[D], 1.0)
        off = _dyadic(rng, D, 2.0)
        if D == 6:
            off[3:] = 0.0
        if D == 3:
            off[2] *= 0.25
        bl = []
        for l in range(K):
            near = 2.0 ** -21 if N == 1 else 1.0                                 # N = 1: every h is the floor, so the points sit within a few floors
            x0 = c.copy(); x0[:NT[D]] += _dyadic(rng, NT[D], 4.0) * near
            if D == 3 and N == 1:                                                 # (N = 2: one shared pair of headings, as for D = 6)
                x0[2] += _dyadic(rng, (), 0.5) * near
            pts = [x0] if N == 1 else [x0, x0 + off]
            if D == 6 and N == 2:
                pts[1][3:] = c[3:] * 0.5                                          # the same two rotations in every proposal
            bl.append(np.array(pts).T.copy())
        blocks.append(bl)
    t = _assemble(D, N, blocks, None, SEED + 3000 + N, 13000 + N, SILVERMAN, rng)
    t["key"], t["want_base"] = key, [0 if len(b) >= 2 else None for b in blocks]
    t["mp_vars"] = [1]
    t["tied"] = [tuple(range(len(b))) if len(b) >= 2 else () for b in blocks]
    return t


FAR_SEPARATIONS = (50.0, 120.0, 300.0, 500.0)


@functools.lru_cache(maxsize=None)
def far_table(D, N=40):
    """two to four proposals whose clusters sit 50 .. 500 bandwidths apart along the first coordinate (supplied bandwidths 0.05·σ): the
    weights of most base particles underflow to exactly 0 and the cumulative weights repeat"""
    key = ("far", D, N, SUPPLIED)
    rng = np.random.default_rng(_seed(key))
    blocks, sigs, bws, want = [], [], [], []
    for v, sep in enumerate(FAR_SEPARATIONS):
        K = 2 + v % 3
        c = _centre(rng, D, edge=False)
        hb = 0.05 * SIG0[D]
        bl, sl, bw = [], [], []
        for l in range(K):
            cl = c.copy(); cl[0] += l * sep * hb[0]
            b, s = _proposal(rng, D, N, cl, 0.05 * (2.0 if l == 0 else 1.0), bimodal=False, edge=False)
            bl.append(b); sl.append(s); bw.append(hb * (0.5 if l == K - 1 else 1.0 + 0.1 * l))
        blocks.append(bl); sigs.append(sl); bws.append(bw); want.append(K - 1)
    t = _assemble(D, N, blocks, sigs, SEED + 4000, 14000, SUPPLIED, rng, bw=bws)
    t["key"], t["want_base"], t["mp_vars"] = key, want, [0, 3]
    return t


def all_tables():
    """(name, table) of every product table, built lazily"""
    for D in DIMS:
        for mode in MODES:
            for N in SHAPE_N[D]:
                yield "shape D=%d N=%d %s" % (D, N, mode), functools.partial(shape_table, D, N, mode)
            for N in LARGE_N:
                yield "large D=%d N=%d %s" % (D, N, mode), functools.partial(large_table, D, N, mode)
        yield "tie D=%d" % D, functools.partial(tie_table, D)
        for N in (1, 2):
            yield "tie D=%d N=%d silverman" % (D, N), functools.partial(small_n_table, D, N)
        yield "far D=%d" % D, functools.partial(far_table, D)


class Reference:
    """Everything the tests need about one product table, computed once and never modified: the noise, np_product of every variable, the
    margins, mp_product of the mp variables (with_mp) and the reference's own error."""

    def __init__(self, t, with_mp=False):
        self.table = t
        D, N = t["D"], t["N"]
        self.V = len(t["ptr"]) - 1
        self.xi = CR.normals(t["seed"], t["stream_offset"], self.V, N, D)
        self.res = np_product(t, self.xi)
        live = [r for r in self.res if r["K"] >= 2]
        self.scale_w = max([1.0] + [r["scale_w"] for r in live])
        self.gap = min([math.inf] + [pick_gap(r) for r in live])
        self.lnh = [lnh_gap(r) for r in live]
        self.zone_margin = math.inf
        if D == 6:
            for r in live:
                r["zone"], r["to_pi"] = zone_of(r["out"]["q"])
                self.zone_margin = min(self.zone_margin, float(np.abs(r["to_pi"] - CR.ZONE_EDGE).min()))
        self.dev = {"c": 0.0, "t": 0.0, "r": 0.0}
        self.mp = {}
        if with_mp:
            with mpm.workdps(DPS):
                for v in t["mp_vars"]:
                    r = self.res[v]
                    m = self.mp[v] = mp_product(t, v, self.xi[v])
                    self.dev["c"] = max(self.dev["c"], max(abs(float(_f(a) - b)) for a, b in zip(r["c"], m["c"])) / r["scale_w"])
                    for i in range(N):
                        et, er = CR._mp_element_distance(KIND[D], _np_as_mp_element(D, r["out"], i), m["out"][i])
                        self.dev["t"] = max(self.dev["t"], float(et) / r["scale_x"])
                        self.dev["r"] = max(self.dev["r"], float(er) / r["scale_x"])

    def delta(self, dev_c):
        return max(8.0 * dev_c, ULP64) * self.scale_w

    def check(self, out, rel_t=ULP64, rel_r=ULP64):
        """kernel output (V, D, N) against every particle of every variable -> (figures, list of failures)"""
        t = self.table
        D, N = t["D"], t["N"]
        out = np.asarray(out)
        bad, fig = [], {"t": 0.0, "r": 0.0, "pick": 0.0, "zone": 0}
        if not np.isfinite(out).all():
            bad.append(("not finite", np.argwhere(~np.isfinite(out))[:4].tolist()))
        for v, r in enumerate(self.res):
            if r["K"] < 2:
                if not np.array_equal(out[v], r["src"]):
                    bad.append(("K = %d block is not a bit copy" % r["K"], v))
                continue
            bt, br = rel_t * r["scale_x"], rel_r * r["scale_x"]
            got = coords_to_elements(D, out[v])
            with np.errstate(all="ignore"):
                et, er = element_distance(D, got, r["out"])
                zone = r.get("zone", np.zeros(N, bool))
                fig["t"] = max(fig["t"], float((et / bt).max())); fig["r"] = max(fig["r"], float(np.where(zone, 0.0, er / br).max()))
                if not ((et <= bt) & ((er <= br) | zone)).all():
                    bad.append(("output", v, np.nonzero(~((et <= bt) & ((er <= br) | zone)))[0][:4].tolist(), float((et / bt).max()),
                                float(np.where(zone, 0.0, er / br).max())))
                if zone.any():                                                    # conv_ref's snap rule
                    fig["zone"] += int(zone.sum())
                    w = out[v][3:].T[zone]
                    nw = np.sqrt(np.sum(w * w, axis=-1))
                    qv = r["out"]["q"][zone][:, 1:]
                    ax = qv / np.sqrt(np.sum(qv * qv, axis=-1))[:, None]
                    da = np.minimum(np.abs(w / nw[:, None] - ax).max(axis=-1), np.abs(w / nw[:, None] + ax).max(axis=-1))
                    if not ((np.abs(nw - math.pi) <= 4.0 * CR.ULP_PI).all() and (da <= br).all()):
                        bad.append(("snap zone", v, float((np.abs(nw - math.pi) / CR.ULP_PI).max()), float((da / br).max())))
                # the pick, recovered from out ⊖ hp⊙ξ: the nearest base particle, which must lie within the output bound.  In the snap zone
                # the output's angle was moved to π (by up to the zone's width), so there the nearest particle alone decides.
                e = r["hp"] * self.xi[v]
                cand = {"t": got["t"] - e[:, :NT[D]]}
                if D == 3:
                    cand["th"] = got["th"] - e[:, 2]
                if D == 6:
                    cand["q"] = q_mul(got["q"], q_conj(q_exp(e[:, 3:])))
                rv = t["rows"][t["ptr"][v]:t["ptr"][v + 1]]
                Pb = coords_to_elements(D, t["prop"][rv[r["base"]]])
                dt, dr = element_distance(D, {k: x[:, None] for k, x in cand.items()}, {k: x[None, :] for k, x in Pb.items()})
                score = np.maximum(dt / bt, dr / br)
                near = score.argmin(axis=1)
                best = score[np.arange(N), near]
                fig["pick"] = max(fig["pick"], float(np.where(zone, 0.0, best).max()))
                wrong = (near != r["picks"]) | (~zone & ~(best <= 1.0))
                if wrong.any():
                    bad.append(("pick", v, np.nonzero(wrong)[0][:6].tolist(), near[wrong][:6].tolist(), r["picks"][wrong][:6].tolist(),
                                float(best.max())))
        return fig, bad


@functools.lru_cache(maxsize=None)
def reference(name, with_mp=False):
    return Reference(dict(all_tables())[name](), with_mp)


# ------------------------------------------------------------------------------------------------------------ belief statistics
STATS_V = 8


@functools.lru_cache(maxsize=None)
def stats_table(D, N):
    """(V, D, N): 0 ordinary; 1 / 2 heading cluster across ±π with particle 0 on either side (D = 6: R₀ within 1e-3 of π, spread 0.1 and
    up to 1 rad); 3 a constant belief; 4 translations at 1e6 with spread 1e-3; 5 bimodal; 6, 7 ordinary far from the origin"""
    rng = np.random.default_rng(8000 + 31 * D + N)
    bel = np.empty((STATS_V, D, N))
    for v in range(STATS_V):
        c = _centre(rng, D, edge=v in (1, 2))
        sig = SIG0[D] * rng.uniform(0.5, 2.0, D)
        e = sig * rng.standard_normal((N, D))
        if v == 1 and D == 3:
            c[2], e[0, 2] = math.pi, -0.02                                        # particle 0 just below +π
        if v == 2 and D == 3:
            c[2], e[0, 2] = math.pi, 0.02                                         # particle 0 just above −π
        if D == 6 and v in (1, 2):
            e[:, 3:] = _unit(rng, (N,)) * rng.uniform(0, 0.1 if v == 1 else 1.0, (N, 1))
            e[0, 3:] = 0.0                                                        # R₀ is the centre: within 1e-3 of π
        if v == 3:
            e[:] = 0.0
        if v == 4:
            c[:NT[D]] = 1e6 * rng.uniform(0.5, 1.0, NT[D]); e[:, :NT[D]] = 1e-3 * rng.standard_normal((N, NT[D]))
        if v == 5:
            e[::2, 0] += 6.0 * sig[0]
        bel[v] = _compose(D, c, e).T
    bel[3] = bel[3][:, :1]                                                        # bit-constant
    return bel


class StatsReference:
    """np_spread of every block of one stats table, its scales, and (with_mp) the deviation from mp_spread on the first six blocks"""

    def __init__(self, D, N, with_mp=False):
        self.D, self.N = D, N
        self.bel = stats_table(D, N)
        self.np = [np_spread(b) for b in self.bel]
        self.scale_d = np.array([max(1.0, float(np.abs(s["d"]).max())) for s in self.np])
        self.scale_m = np.maximum(self.scale_d, np.abs(self.bel).max(axis=(1, 2)))
        self.sd = np.array([s["sd"] for s in self.np])
        self.mean = {k: np.array([s[k] for s in self.np]) for k in ("t",) + (("th",) if D == 3 else ("q",) if D == 6 else ())}
        self.zone_margin = math.inf
        if D == 6:
            zone, to_pi = zone_of(self.mean["q"])
            self.zone_margin = float((to_pi - CR.ZONE_EDGE).min())                # every mean stays OUTSIDE the snap zone of so3_log
        self.dev = {"t": 0.0, "r": 0.0, "sd": 0.0}
        if with_mp:
            with mpm.workdps(DPS):
                for v in range(6):
                    mean, sd, _ = mp_spread(self.bel[v])
                    et, er = CR._mp_element_distance(KIND[D], _np_as_mp_element(D, self.mean, v), mean)
                    self.dev["t"] = max(self.dev["t"], float(et) / self.scale_m[v]); self.dev["r"] = max(self.dev["r"], float(er) / self.scale_m[v])
                    self.dev["sd"] = max(self.dev["sd"], max(abs(float(_f(a) - b)) for a, b in zip(self.sd[v], sd)) / self.scale_d[v])

    def check(self, mean, sd, rel=ULP64, rel_r=None):
        """mean / sd (V, D) -> (figures, failures); rel_r: another relative bound for the rotation part of the mean alone"""
        D = self.D
        got = coords_to_elements(D, np.asarray(mean).T)
        et, er = element_distance(D, got, self.mean)
        es = np.abs(np.asarray(sd) - self.sd).max(axis=1)
        bm, bs = rel * self.scale_m, rel * self.scale_d
        br = bm if rel_r is None else rel_r * self.scale_m
        fig = {"t": float((et / bm).max()), "r": float((er / br).max()), "sd": float((es / bs).max())}
        bad = [(k, np.nonzero(~(x <= b))[0].tolist(), fig[k]) for k, x, b in (("t", et, bm), ("r", er, br), ("sd", es, bs)) if not (x <= b).all()]
        if not np.array_equal(np.asarray(sd)[3, :NT[D] + (D == 3)], np.zeros(NT[D] + (D == 3))):
            bad.append(("constant belief: sd is not exactly 0", np.asarray(sd)[3].tolist()))
        if D == 6 and not (np.asarray(sd)[3, 3:] <= bs[3]).all():
            bad.append(("constant belief: rotation sd", np.asarray(sd)[3].tolist()))
        nexact = D if D < 6 else 3
        if not np.array_equal(np.asarray(mean)[3, :nexact], self.bel[3, :nexact, 0]):
            bad.append(("constant belief: the mean is not the point", np.asarray(mean)[3].tolist()))
        return fig, bad


@functools.lru_cache(maxsize=None)
def stats_reference(D, N, with_mp=False):
    return StatsReference(D, N, with_mp)
