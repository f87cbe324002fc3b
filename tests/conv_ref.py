"""References for the convolution ROOTS of the unique-root factors (Pose2Pose2 + PriorPose2 rows, bearing-range -> landmark, Pose3Pose3 +
PriorPose3 rows): what the packed sweep k_conv_flat, the wave-per-row k_conv and k_conv_big must return for every particle of a table.

Three sides, none of which is the kernel:
  * mp_root  -- mpmath at lin_ref.DPS digits on GROUP ELEMENTS (headings / rotation matrices through lin_ref's primitives), one particle.
  * np_root  -- float64 NumPy over a whole table; SE(3) on unit quaternions written the plain way (Exp by sin(θ/2)/θ, angles by atan2).
                It never forms a matrix logarithm.
  * the C oracle, in tests/test_conv_ref_host.py only: it ties the noise plumbing and the row conventions of np_root to ro.conv_*.

Noise.  Row c of a table, particle i, draws ξ = ro.rng_normals(seed, stream_offset + c, i, dz): the stream is the table's stream_offset plus
the ROW index (not the factor index), the particle id is the particle's index in its belief block.  rng_normals itself pairs particles
2j / 2j + 1 on one Philox call (pinned on known answers in tests/test_host_logic.py); nothing here depends on N or on the launch shape.
The measurement is z = μ + Lξ with L the packed lower Cholesky factor (row-major lower triangle), bearing-range: z = μ + σ∘ξ.

Comparison.  `distance` compares GROUP ELEMENTS: translation error (largest component) and rotation error (Pose2: wrapped heading
difference; Pose3: the angle of Refᵀ·Exp(ω_out)).  The conditioning of the logarithm near π and the ω <-> −(2π − |ω|)·axis ambiguity
are thereby not part of the comparison.

Bounds (class Reference; nothing comes from a GPU run).  Per table and part: dev = largest deviation of np_root from mp_root on the mp
rows relative to the row scale, where the row scale of the translation part is max(1, largest |translation coordinate| of the row: fixed
particles, μ_t (bearing-range: μ_ρ), root) and that of the rotation part max(1, largest |angle coordinate|: fixed headings / rotation
vectors, μ_θ / μ_ω).  The kernel's bound is max(8·dev, 64 ulp) x row scale -- the margin of lin_ref.Reference, a correct double
evaluation in another operation order -- plus √d·tol under GAUSS_NEWTON (d = 3, 2, 6): a point accepted at max|r| <= tol lies within
‖r‖₂ <= √d·tol of the unique root in its tangent coordinates.

Snap zone (Pose3 only).  quat_log returns θ = π exactly where 2·q_w² <= √eps (as Manifolds' log does, rome_device_math.hpp), i.e. for
true angles within acos(1 − √eps) = 1.7263e-4 of π.  The REFERENCE decides membership from its own q_w; for those particles the rule
is |‖ω_out‖ − π| <= 4 ulp(π) and axis_out = ±axis_ref within the table's rotation bound.  Every table keeps all particles at least 1e-5
(in angle) from the zone's edge (checked on the CPU), so that membership cannot tie.

Measured dev (CPU, this file's tables; printed by tests/test_conv_ref_host.py -s), in units of eps = 2^-52, translation / rotation:
  shape tables, all N      Pose2Pose2 <= 2.07 / 1.58    bearing-range <= 2.35 / --     Pose3Pose3 <= 1.71 / 1.71
  edge tables              Pose2Pose2    0.86 / 0.94    bearing-range    2.04 / --     Pose3Pose3    2.93 / 1.42
Every 8·dev lies below the floor, so every bound is the floor: 64 ulp = 1.42e-14 times the row scale (+ √d·tol under GAUSS_NEWTON).
tests/test_conv_ref_host.py holds dev under 8 eps, so a table cannot move a bound without failing there first.
"""
import ctypes as C
import functools
import math

import mpmath as mpm
import numpy as np

import lin_ref as L
from lin_ref import DPS, EPS, SQRT_EPS, _mm, _mt, _mv, _rot2, _so3_exp, _so3_log, _wrap   # noqa: F401  (the mp primitives, shared)

P2P2, BR0, P3P3 = "p2p2", "br0", "p3p3"
KINDS = (P2P2, BR0, P3P3)
NAMES = {P2P2: "Pose2Pose2", BR0: "Pose2Point2BearingRange->landmark", P3P3: "Pose3Pose3"}
DIMS = {P2P2: (3, 3, 3, 6), BR0: (2, 3, 2, 2), P3P3: (6, 6, 6, 21)}            # dz, df (fixed), dt (target), doubles of L per factor
GN_DIM = {P2P2: 3, BR0: 2, P3P3: 6}
DIR_PRIOR = 2
SEED = 0x524F4D45
ULP64 = 64.0 * EPS
ZONE_EDGE = math.acos(1.0 - SQRT_EPS)         # π − θ at 2 q_w² = 1 + cos θ = √eps: 1.7263e-4
ZONE_MARGIN = 1e-5
ULP_PI = 2.0 ** -51                            # spacing of doubles in [2, 4)

# ------------------------------------------------------------------------------------------------------------ launch arithmetic
FLAT_THREADS, FLAT_MAX_ROWS, FLAT_MIN_N = 256, 16, 16     # kFlatThreads, kFlatMaxRows, the N >= 16 test of launch_ppl


def launch_shape(N, n_conv):
    """the packed sweep's launch (launch_flat): pair-threads per row H, rows per block CPB, blocks nb, live threads of a full block,
    whether the CPB clamp acted"""
    H = (N + 1) // 2
    if N < FLAT_MIN_N or H > FLAT_THREADS:       # k_conv / k_conv_big: one wavefront per row, four rows per block
        return {"H": 64, "CPB": 4, "nb": -(-n_conv // 4), "live": 256, "clamped": False, "packed": False}
    raw = FLAT_THREADS // H
    CPB = min(FLAT_MAX_ROWS, raw)
    return {"H": H, "CPB": CPB, "nb": -(-n_conv // CPB), "live": CPB * H, "clamped": raw > FLAT_MAX_ROWS,
            "packed": N >= FLAT_MIN_N and H <= FLAT_THREADS}


# N -> the case it is listed for, as a predicate on launch_shape (tests/test_conv_ref_host.py asserts each)
SHAPE_CASES = {
    16: ("CPB at the clamp, half the block dead", lambda s: s["clamped"] and s["CPB"] == 16 and s["live"] == 128),
    17: ("clamp, odd tail", lambda s: s["clamped"] and s["CPB"] == 16 and s["live"] < 256),
    30: ("clamp, last thread slots dead", lambda s: s["clamped"] and s["CPB"] == 16 and s["live"] == 240),
    32: ("a full block exactly, no clamp", lambda s: not s["clamped"] and s["CPB"] == 16 and s["live"] == 256),
    34: ("one dead slot with lc_raw == CPB", lambda s: s["live"] == 255 and 255 // s["H"] == s["CPB"] == 15),
    100: ("CPB = 5", lambda s: s["CPB"] == 5 and s["H"] == 50),
    101: ("CPB = 5, odd tail", lambda s: s["CPB"] == 5 and s["H"] == 51),
    170: ("CPB = 3, one dead slot with lc_raw == CPB", lambda s: s["CPB"] == 3 and s["live"] == 255 and 255 // s["H"] == 3),
    172: ("CPB = 2", lambda s: s["CPB"] == 2 and s["live"] == 172),
    256: ("CPB = 2, full block", lambda s: s["CPB"] == 2 and s["live"] == 256),
    258: ("CPB = 1", lambda s: s["CPB"] == 1 and s["H"] == 129),
    511: ("CPB = 1, odd tail, H = 256", lambda s: s["CPB"] == 1 and s["H"] == 256),
    512: ("CPB = 1, the upper end of the packed range", lambda s: s["CPB"] == 1 and s["live"] == 256),
}
PACKED_N = tuple(SHAPE_CASES)
NEIGHBOUR_N = (15, 513)                      # k_conv (one particle per lane) and k_conv_big: the two neighbours that leave the packed kernel
NB = (1, 7, 8, 9, 19)


def n_conv_list(kind, N):
    """n_conv per block count of NB; where CPB > 1 the last block is partly filled.  Pose3 at N >= 256: the three smallest."""
    s = launch_shape(N, 1)
    nbs = NB[:3] if (kind == P3P3 and N >= 256) else NB
    return [(nb - 1) * s["CPB"] + max(1, s["CPB"] // 2) for nb in nbs]


# ------------------------------------------------------------------------------------------------------------ noise
def normals(seed, stream_offset, n_conv, N, dz):
    """ξ[c, i, :] = ro.rng_normals(seed, stream_offset + c, i, dz) (one ctypes call per particle, the buffer reused)"""
    import oracle as ro
    fn = ro.lib().ro_rng_normals
    buf = np.zeros(dz + 1)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    out = np.empty((n_conv, N, dz))
    sd = C.c_uint64(seed)
    for c in range(n_conv):
        st = C.c_uint64(stream_offset + c)
        for i in range(N):
            fn(sd, st, C.c_uint32(i), dz, p)
            out[c, i] = buf[:dz]
    return out


# ------------------------------------------------------------------------------------------------------------ float64 quaternions
def q_exp(w):
    """Exp(ω) = (cos θ/2, sin(θ/2)/θ · ω), θ = ‖ω‖ (θ = 0: ½ ω)"""
    th = np.sqrt(np.sum(w * w, axis=-1))
    nz = th > 0.0
    k = np.where(nz, np.sin(0.5 * th) / np.where(nz, th, 1.0), 0.5)
    return np.concatenate([np.cos(0.5 * th)[..., None], k[..., None] * w], axis=-1)


def q_conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def q_mul(a, b):
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return np.concatenate([aw * bw - np.sum(av * bv, axis=-1, keepdims=True), aw * bv + bw * av + np.cross(av, bv)], axis=-1)


def q_rot(q, v):
    """R(q) v = v + 2 w (u x v) + 2 u x (u x v)"""
    u = q[..., 1:]
    t = 2.0 * np.cross(u, v)
    return v + q[..., :1] * t + np.cross(u, t)


def q_angle(q):
    """rotation angle in [0, π]: 2 atan2(‖vec‖, |w|)"""
    return 2.0 * np.arctan2(np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1)), np.abs(q[..., 0]))


def q_log(q):
    """principal rotation vector of ±q (no snap)"""
    n = np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1))
    w = q[..., 0]
    nz = n > 0.0
    k = np.where(nz, 2.0 * np.arctan2(n, np.abs(w)) / np.where(nz, n, 1.0), 2.0 / np.where(w == 0.0, 1.0, np.abs(w)))
    return (np.where(w < 0.0, -k, k))[..., None] * q[..., 1:]


def _np_remainder(x):
    return np.vectorize(math.remainder, otypes=[np.float64])(x, 2.0 * math.pi)


# ------------------------------------------------------------------------------------------------------------ tables
def _lower(kind, Lp):
    """packed rows of L -> (F, dz, dz) lower-triangular (bearing-range: diag σ)"""
    dz = DIMS[kind][0]
    F = len(Lp)
    M = np.zeros((F, dz, dz))
    if kind == BR0:
        M[:, 0, 0] = Lp[:, 0]; M[:, 1, 1] = Lp[:, 1]
    else:
        r, c = np.tril_indices(dz)
        M[:, r, c] = Lp
    return M


def measurements(t, xi):
    """z[c, i, :] = μ_f + L_f ξ in float64, in the kernel's summation order (left to right along a row of L)"""
    f = t["rows4"][:, 0]
    Lf = _lower(t["kind"], t["L"])[f]
    z = np.array(np.broadcast_to(t["mu"][f][:, None, :], xi.shape))
    for j in range(xi.shape[2]):
        z = z + Lf[:, None, :, j] * xi[:, :, j:j + 1]
    return z


def np_root(t, xi):
    """the root of every particle of every row -> {"t": (C, N, 2|3), "th": (C, N) | "q": (C, N, 4)} (bearing-range: "t" only)"""
    kind = t["kind"]
    z = measurements(t, xi)
    rows = t["rows4"]
    fx = np.swapaxes(t["bel_fixed"][rows[:, 2]], 1, 2)                        # (C, N, df)
    d = rows[:, 1][:, None]
    if kind == BR0:
        a = fx[..., 2] + z[..., 0]
        return {"t": fx[..., :2] + z[..., 1:2] * np.stack([np.cos(a), np.sin(a)], -1)}
    if kind == P2P2:
        pr, back = d == DIR_PRIOR, d == 1
        th = np.where(pr, z[..., 2], np.where(back, fx[..., 2] - z[..., 2], fx[..., 2] + z[..., 2]))
        rot = np.where(pr, 0.0, np.where(back, th, fx[..., 2]))               # the frame z_t is turned by
        c, s = np.cos(rot), np.sin(rot)
        v = np.stack([c * z[..., 0] - s * z[..., 1], s * z[..., 0] + c * z[..., 1]], -1)
        base = np.where(pr[..., None], 0.0, fx[..., :2])
        return {"t": np.where(back[..., None], base - v, base + v), "th": th}
    qz, qF = q_exp(z[..., 3:]), q_exp(fx[..., 3:])
    pr, back = (d == DIR_PRIOR)[..., None], (d == 1)[..., None]
    q = np.where(pr, qz, np.where(back, q_mul(qF, q_conj(qz)), q_mul(qF, qz)))
    v = q_rot(np.where(back, q, qF), z[..., :3])
    tt = np.where(pr, z[..., :3], np.where(back, fx[..., :3] - v, fx[..., :3] + v))
    return {"t": tt, "q": q}


def root_coords(kind, root):
    """(C, dt, N) SoA coordinates of a root: the start points of the mixed-convergence tables"""
    if kind == BR0:
        return np.swapaxes(root["t"], 1, 2).copy()
    last = root["th"][..., None] if kind == P2P2 else q_log(root["q"])
    return np.swapaxes(np.concatenate([root["t"], last], -1), 1, 2).copy()


# ------------------------------------------------------------------------------------------------------------ mpmath side
def _f(v):
    return mpm.mpf(float(v))


def mp_root(kind, dr, mu, Lp, xi, fixed):
    """one particle at the current mp precision; float64 inputs taken exactly.  Lp: the factor's packed L (bearing-range: σ).
    -> (t, θ) Pose2, (l,) landmark, (t, R) Pose3"""
    dz = DIMS[kind][0]
    M = _lower(kind, np.asarray(Lp, dtype=np.float64)[None])[0]
    z = [_f(mu[k]) + sum(_f(M[k, j]) * _f(xi[j]) for j in range(dz)) for k in range(dz)]
    fx = [_f(v) for v in fixed]
    if kind == BR0:
        a = fx[2] + z[0]
        return ([fx[0] + z[1] * mpm.cos(a), fx[1] + z[1] * mpm.sin(a)],)
    if kind == P2P2:
        if dr == DIR_PRIOR:
            return (z[:2], z[2])
        if dr == 0:
            v = _mv(_rot2(fx[2]), z[:2])
            return ([fx[0] + v[0], fx[1] + v[1]], fx[2] + z[2])
        th = fx[2] - z[2]
        v = _mv(_rot2(th), z[:2])
        return ([fx[0] - v[0], fx[1] - v[1]], th)
    Z = _so3_exp(z[3:])
    if dr == DIR_PRIOR:
        return (z[:3], Z)
    RF = _so3_exp(fx[3:])
    if dr == 0:
        v = _mv(RF, z[:3])
        return ([fx[k] + v[k] for k in range(3)], _mm(RF, Z))
    Rp = _mm(RF, _mt(Z))
    v = _mv(Rp, z[:3])
    return ([fx[k] - v[k] for k in range(3)], Rp)


def _mp_angle(U):
    """rotation angle of U in [0, π]: atan2(‖skew part‖, trace part)"""
    v = [(U[2][1] - U[1][2]) / 2, (U[0][2] - U[2][0]) / 2, (U[1][0] - U[0][1]) / 2]
    return mpm.atan2(mpm.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), (U[0][0] + U[1][1] + U[2][2] - 1) / 2)


def _mp_quat_matrix(q):
    """R of a (nearly unit) float64 quaternion, exactly: I + 2 (w K + K²)/|q|²"""
    w, x, y, z = [_f(v) for v in q]
    n = w * w + x * x + y * y + z * z
    K = [[0, -z, y], [z, 0, -x], [-y, x, 0]]
    K2 = _mm(K, K)
    return [[mpm.mpf(i == j) + 2 * (w * K[i][j] + K2[i][j]) / n for j in range(3)] for i in range(3)]


def _mp_element_distance(kind, a, b):
    """(translation error, rotation error) between two mp group elements"""
    et = max(abs(x - y) for x, y in zip(a[0], b[0]))
    if kind == BR0:
        return et, mpm.mpf(0)
    if kind == P2P2:
        return et, abs(_wrap(a[1] - b[1]))
    return et, _mp_angle(_mm(_mt(b[1]), a[1]))


def distance(kind, out, ref, mp=False):
    """out: coordinates.  float64 (mp=False): out (C, dt, N) against ref = np_root's dict -> (et, er) arrays (C, N).
    mp=True: out = the dt coordinates of ONE particle, ref = mp_root's element -> (et, er) mpf."""
    if mp:
        o = [_f(v) for v in out]
        if kind == BR0:
            el = (o,)
        elif kind == P2P2:
            el = (o[:2], o[2])
        else:
            el = (o[:3], _so3_exp(o[3:]))
        return _mp_element_distance(kind, el, ref)
    o = np.swapaxes(np.asarray(out), 1, 2)
    nt = ref["t"].shape[-1]
    et = np.abs(o[..., :nt] - ref["t"]).max(axis=-1)
    if kind == BR0:
        return et, np.zeros_like(et)
    if kind == P2P2:
        return et, np.abs(_np_remainder(o[..., 2] - ref["th"]))
    return et, q_angle(q_mul(q_conj(ref["q"]), q_exp(o[..., 3:])))


def mp_rows_of(t):
    """the rows the mp side serves: every edge row plus a seeded 5 % (at least one) of the random rows"""
    n = t["n_conv"]
    edge = sorted(t.get("edge_rows", ()))
    rnd = [c for c in range(n) if c not in set(edge)]
    k = max(1, int(math.ceil(0.05 * len(rnd)))) if rnd else 0
    pick = np.random.default_rng(900 + n + t["N"]).choice(len(rnd), size=k, replace=False) if k else []
    return sorted(set(edge) | {rnd[int(j)] for j in pick})


class Reference:
    """Everything the tests need about one table, computed once and never modified: the noise, the float64 root of every particle, the
    mp root of the mp rows, the measured reference error and the bounds."""

    def __init__(self, t):
        kind = self.kind = t["kind"]
        self.table = t
        Cn, N = t["n_conv"], t["N"]
        rows = t["rows4"]
        self.xi = normals(t["seed"], t["stream_offset"], Cn, N, DIMS[kind][0])
        with np.errstate(all="ignore"):
            self.root = np_root(t, self.xi)
        fx = t["bel_fixed"][rows[:, 2]]                                        # (C, df, N)
        prior = rows[:, 1] == DIR_PRIOR if kind != BR0 else np.zeros(Cn, bool)
        nt = 3 if kind == P3P3 else 2
        fxt = np.where(prior[:, None], 0.0, np.abs(fx[:, :nt]).max(axis=(1, 2))[:, None])[:, 0]
        mu_f = np.abs(t["mu"][rows[:, 0]])
        mu_t = mu_f[:, 1] if kind == BR0 else mu_f[:, :nt].max(axis=1)
        self.scale_t = np.maximum(1.0, np.maximum.reduce([fxt, mu_t, np.abs(self.root["t"]).max(axis=(1, 2))]))
        fxr = np.where(prior, 0.0, np.abs(fx[:, nt:]).max(axis=(1, 2)))
        mu_r = mu_f[:, 0] if kind == BR0 else mu_f[:, nt:].max(axis=1)
        self.scale_r = np.maximum(1.0, np.maximum(fxr, mu_r))
        if kind == P3P3:
            q = self.root["q"]
            self.qw2 = 2.0 * q[..., 0] ** 2 / np.sum(q * q, axis=-1)
            self.zone = self.qw2 <= SQRT_EPS
            self.to_pi = 2.0 * np.arctan2(np.abs(q[..., 0]), np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1)))   # π − θ, accurate near π
        else:
            self.zone = np.zeros((Cn, N), bool)
        # ---- mp rows, the reference's own error
        self.rows = mp_rows_of(t)
        self.mp = {}
        dev_t = dev_r = 0.0
        with mpm.workdps(DPS):
            for c in self.rows:
                f, dr, fv = int(rows[c, 0]), int(rows[c, 1]), int(rows[c, 2])
                els = []
                for i in range(N):
                    el = mp_root(kind, dr, t["mu"][f], t["L"][f], self.xi[c, i], t["bel_fixed"][fv, :, i])
                    els.append(el)
                    if kind == BR0:
                        mine = ([_f(v) for v in self.root["t"][c, i]],)
                    elif kind == P2P2:
                        mine = ([_f(v) for v in self.root["t"][c, i]], _f(self.root["th"][c, i]))
                    else:
                        mine = ([_f(v) for v in self.root["t"][c, i]], _mp_quat_matrix(self.root["q"][c, i]))
                    et, er = _mp_element_distance(kind, mine, el)
                    dev_t = max(dev_t, float(et) / self.scale_t[c]); dev_r = max(dev_r, float(er) / self.scale_r[c])
                self.mp[c] = els
        self.dev = {"t": dev_t, "r": dev_r}
        self.rel_bound = {k: max(8.0 * v, ULP64) for k, v in self.dev.items()}

    def bounds(self, gn_tol=0.0, n=None):
        """per-row bounds (n,) of the translation and the rotation part; gn_tol: the tolerance GAUSS_NEWTON ran with (0: the closed form)"""
        add = math.sqrt(GN_DIM[self.kind]) * gn_tol
        return self.rel_bound["t"] * self.scale_t[:n] + add, self.rel_bound["r"] * self.scale_r[:n] + add

    def check(self, out, gn_tol=0.0, mp=False):
        """kernel output (n, dt, N), n <= n_conv rows of the table from row 0, against the float64 root of EVERY particle (and, mp=True,
        against mp on the mp rows) -> dict of the worst figures, each as a fraction of its bound (<= 1 passes), and a list of failures"""
        out = np.asarray(out)
        n = out.shape[0]
        bt, br = self.bounds(gn_tol, n)
        ref = {k: v[:n] for k, v in self.root.items()}
        zone = self.zone[:n]
        with np.errstate(all="ignore"):
            et, er = distance(self.kind, out, ref)
        fig = {"t": float((et / bt[:, None]).max()), "r": float(np.where(zone, 0.0, er / br[:, None]).max()), "zone": int(zone.sum())}
        bad = []
        if not fig["t"] <= 1.0:
            bad.append(("translation", np.argwhere(~(et <= bt[:, None]))[:4].tolist(), fig["t"]))
        if not fig["r"] <= 1.0:
            bad.append(("rotation", np.argwhere(~((er <= br[:, None]) | zone))[:4].tolist(), fig["r"]))
        if zone.any():                                                          # the snap rule
            w = np.swapaxes(out, 1, 2)[..., 3:][zone]
            nw = np.sqrt(np.sum(w * w, axis=-1))
            qv = ref["q"][zone][:, 1:]
            ax = qv / np.sqrt(np.sum(qv * qv, axis=-1))[:, None]
            ao = w / nw[:, None]
            da = np.minimum(np.abs(ao - ax).max(axis=-1), np.abs(ao + ax).max(axis=-1))
            fig["zone_norm_ulp"] = float((np.abs(nw - math.pi) / ULP_PI).max())
            fig["zone_axis"] = float((da / np.broadcast_to(br[:, None], zone.shape)[zone]).max())
            if not fig["zone_norm_ulp"] <= 4.0:
                bad.append(("snap zone: |ω| is not π", fig["zone_norm_ulp"]))
            if not fig["zone_axis"] <= 1.0:
                bad.append(("snap zone: axis", fig["zone_axis"]))
        if mp:
            worst_t = worst_r = 0.0
            with mpm.workdps(DPS):
                for c in self.rows:
                    if c >= n:
                        continue
                    for i in range(self.table["N"]):
                        mt, mr = distance(self.kind, out[c, :, i], self.mp[c][i], mp=True)
                        worst_t = max(worst_t, float(mt) / bt[c])
                        if not zone[c, i]:
                            worst_r = max(worst_r, float(mr) / br[c])
            fig["mp_t"], fig["mp_r"] = worst_t, worst_r
            if not (worst_t <= 1.0 and worst_r <= 1.0):
                bad.append(("against mp", worst_t, worst_r))
        return fig, bad


# ------------------------------------------------------------------------------------------------------------ case tables
def _unit(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def _chol_rows(rng, F, dz, scales):
    """packed lower-triangular factors with the given diagonal scales and small off-diagonal entries"""
    M = np.zeros((F, dz, dz))
    for k in range(dz):
        M[:, k, k] = scales[k] * rng.uniform(0.5, 1.5, F)
        for j in range(k):
            M[:, k, j] = 0.2 * scales[k] * rng.standard_normal(F)
    r, c = np.tril_indices(dz)
    return M[:, r, c]


def shape_table(kind, N, stream_offset=None, own_targets=False, n_conv=None):
    """The mixed table of one (family, N): n_conv rows for 19 blocks (the smaller launches take its first rows).  The factor index differs
    from the row index with repeats (F = 7 < n_conv), fixed and target variables are out of order and every variable is fixed in several
    rows, dir 0 / dir 1 / prior rows are interleaved (c mod 3).  Translations within ±50 (the status tests evaluate the functor against an
    absolute 1e-12), Pose3 rotations small enough that no root comes near π by accident (|p_ω| <= 1.3, |μ_ω| <= 1, σ_ω = 0.05).
    own_targets: every row gets a target variable of its own (the mixed-convergence tables write per-row start points)."""
    dz, df, dt, nl = DIMS[kind]
    n_conv = max(n_conv_list(kind, N)) if n_conv is None else n_conv
    rng = np.random.default_rng(5000 + 97 * KINDS.index(kind) + N)
    F, V = 7, 11
    c = np.arange(n_conv)
    rows = np.stack([(5 * c + 3) % F, c % 3 if kind != BR0 else np.zeros_like(c), (7 * c + 2) % V, (3 * c + 5) % V], 1).astype(np.int32)
    if stream_offset is None:
        stream_offset = (1 << 32) + 12345 if N == 100 else 1000 + N          # above 2^32 once per family
    t = {"kind": kind, "N": N, "n_conv": n_conv, "seed": SEED + N, "stream_offset": stream_offset, "edge_rows": ()}
    if kind == P3P3:
        t["mu"] = np.concatenate([rng.uniform(-5, 5, (F, 3)), _unit(rng, (F,)) * rng.uniform(0, 1.0, (F, 1))], 1)
        t["L"] = _chol_rows(rng, F, 6, [0.3, 0.3, 0.3, 0.05, 0.05, 0.05])
        bel = np.concatenate([rng.uniform(-40, 40, (V, 3, 1)) + rng.standard_normal((V, 3, N)),
                              np.swapaxes(_unit(rng, (V, N)) * rng.uniform(0, 1.3, (V, N, 1)), 1, 2)], 1)
    else:
        if kind == P2P2:
            t["mu"] = rng.uniform(-5, 5, (F, 3)) * [1, 1, 0.6]
            t["L"] = _chol_rows(rng, F, 3, [0.3, 0.3, 0.1])
        else:
            t["mu"] = np.stack([rng.uniform(-3.1, 3.1, F), rng.uniform(2.0, 20.0, F)], 1)
            t["L"] = np.stack([rng.uniform(0.01, 0.1, F), rng.uniform(0.05, 0.25, F)], 1)      # μ_ρ >= 8 σ_ρ
        bel = rng.uniform(-40, 40, (V, 3, 1)) * np.array([1, 1, 0])[None, :, None] + rng.standard_normal((V, 3, N)) * np.array([1, 1, 0.3])[None, :, None]
        bel[:, 2] += rng.uniform(-math.pi, math.pi, (V, 1))
        bel[:, 2] = np.arctan2(np.sin(bel[:, 2]), np.cos(bel[:, 2]))
    t["bel_fixed"] = bel
    if kind == BR0:
        t["bel_target"] = rng.uniform(-40, 40, (V, 2, 1)) + rng.standard_normal((V, 2, N))
    if own_targets:
        start = rng.uniform(-40, 40, (n_conv, dt, 1)) + rng.standard_normal((n_conv, dt, N))
        if kind == P3P3:
            start[:, 3:] = np.swapaxes(_unit(rng, (n_conv, N)) * rng.uniform(0, 2.5, (n_conv, N, 1)), 1, 2)
        if kind == BR0:
            t["bel_target"] = start
            rows[:, 3] = c
        else:
            t["bel_fixed"] = np.concatenate([bel, start], 0)
            rows[:, 3] = V + c
    t["rows4"] = rows
    t["mu"] = np.ascontiguousarray(t["mu"], dtype=np.float64)
    return t


P3_MAGS = (0.0, 1e-12, 0.9e-8, 1.1e-8, 1e-4, 1.0, 3.0, math.pi - 1e-2, math.pi - 1e-3, math.pi - 3e-4,
           math.pi - 1e-4, math.pi - 1e-6,                                    # inside the snap zone
           4.0)                                                               # beyond the principal range
P3_TRANSLATIONS = (1e-3, 1.0, 1e6)
EDGE_N = 34                                                                   # H = 17 < NK = 27: two staging passes; the dead slot lc_raw == CPB
N_EDGE_FILL = 40                                                              # ordinary rows behind the edge rows (keeps the snap zone under 5 % of the table)


class _Builder:
    """collects rows with a factor and variables of their own; the table's row order is then shuffled by a fixed permutation"""

    def __init__(self, kind, N, seed):
        self.kind, self.N = kind, N
        self.rng = np.random.default_rng(seed)
        self.mu, self.L, self.bel, self.rows, self.edge = [], [], [], [], []

    def var(self, block):
        self.bel.append(np.asarray(block, dtype=np.float64)); return len(self.bel) - 1

    def row(self, dr, mu, Lp, fixed_block, target=None, edge=True):
        self.mu.append(np.asarray(mu, dtype=np.float64)); self.L.append(np.asarray(Lp, dtype=np.float64))
        fv = self.var(fixed_block)
        self.rows.append([len(self.mu) - 1, dr, fv, fv if target is None else target])
        self.edge.append(edge)
        return len(self.rows) - 1

    def table(self, stream_offset):
        n = len(self.rows)
        perm = np.random.default_rng(77).permutation(n)                        # factor / variable indices end up out of row order
        rows = np.array(self.rows, dtype=np.int32)[perm]
        return {"kind": self.kind, "N": self.N, "n_conv": n, "seed": SEED + 7, "stream_offset": stream_offset,
                "mu": np.array(self.mu), "L": np.array(self.L), "bel_fixed": np.array(self.bel), "rows4": rows,
                "edge_rows": tuple(int(k) for k in np.nonzero(np.array(self.edge)[perm])[0])}


def _diagL(dz, diag):
    M = np.zeros((dz, dz)); M[np.arange(dz), np.arange(dz)] = diag
    r, c = np.tril_indices(dz)
    return M[r, c]


def pose3_edge_table():
    """The SE(3) angle edges, N = 34.  Per magnitude m of P3_MAGS five rows: (a) dir 0 and (b) dir 1 with the FIXED rotation vectors
    m·axis_i (p_ω and q_ω: a random unit axis per particle, the first three particles on the coordinate axes), (c) dir 0 and (d) dir 1
    with μ_ω = m·axis and a tiny Σ_ω against an ordinary fixed pose, (e) a prior row with the same μ_ω.  Σ_ω is 1e-3·m on the diagonal (1e-9 at most; exactly 0 for m = 0), so |z_ω| stays on its side of the
    th2 > 1e-16 switch and 1e-5 clear of the snap zone's edge.  The target variable of a row is the fixed block of the next magnitude:
    GAUSS_NEWTON starts from every magnitude as well, the zone and 4.0 included.  Then the compositions on one axis (2 + 2 > π; a sum
    inside the zone; p and z cancelling to the identity; each in dir 0 and dir 1), the translation scales, and ordinary rows."""
    N = EDGE_N
    b = _Builder(P3P3, N, 6100)
    rng = b.rng

    def axes():
        a = _unit(rng, (N,)); a[:3] = np.eye(3); return a

    def pose_block(omega, tscale=3.0):
        return np.concatenate([rng.standard_normal((3, N)) * tscale, np.asarray(omega).T], 0)
    Lmod = _chol_rows(rng, 1, 6, [0.3, 0.3, 0.3, 0.05, 0.05, 0.05])[0]
    first = {}
    for k, m in enumerate(P3_MAGS):
        ax = _unit(rng, ())
        if k % 3 == 0:
            ax = np.eye(3)[k % 2]
        sw = min(1e-9, 1e-3 * m)
        Ltiny = _diagL(6, [0.3, 0.3, 0.3, sw, sw, sw])
        mu_mod = np.concatenate([rng.standard_normal(3) * 2, _unit(rng, ()) * 0.7])
        mu_edge = np.concatenate([rng.standard_normal(3) * 2, m * ax])
        first[k] = b.row(0, mu_mod, Lmod, pose_block(m * axes()))                                        # p_ω = m
        b.row(1, mu_mod * np.array([1, 1, 1, -1, -1, -1.0]), Lmod, pose_block(m * axes()))               # q_ω = m
        for dr in (0, 1):                                                                                # z_ω = m against an ordinary pose
            b.row(dr, mu_edge, Ltiny, pose_block(_unit(rng, (N,)) * rng.uniform(0.2, 1.2, (N, 1))))
        b.row(DIR_PRIOR, mu_edge, Ltiny, pose_block(np.zeros((N, 3))))
    for k in range(len(P3_MAGS)):                                              # start points: the fixed block of the next magnitude
        b.rows[first[k]][3] = b.rows[first[(k + 1) % len(P3_MAGS)]][2]
    ax = np.array([0.36, -0.48, 0.8])
    for dr in (0, 1):
        sg = 1.0 if dr == 0 else -1.0                                          # dir 1 composes with Exp(z)ᵀ
        comps = ((2.0, 2.0, 0.0), (2.0, math.pi - 2.0 - 5e-5, 1e-9), (1.3, -1.3, 0.0))
        for pa, za, sw in comps:
            b.row(dr, np.concatenate([rng.standard_normal(3), sg * za * ax]), _diagL(6, [0.3, 0.3, 0.3, sw, sw, sw]),
                  pose_block(np.tile(pa * ax, (N, 1))))
    for s in P3_TRANSLATIONS:
        for dr in (0, 1, DIR_PRIOR):
            mu = np.concatenate([rng.standard_normal(3) * s, _unit(rng, ()) * 0.8])
            b.row(dr, mu, _diagL(6, [0.1 * s] * 3 + [0.05] * 3), pose_block(_unit(rng, (N,)) * rng.uniform(0, 1.2, (N, 1)), tscale=s))
    for k in range(N_EDGE_FILL):
        mu = np.concatenate([rng.standard_normal(3) * 2, _unit(rng, ()) * rng.uniform(0, 1.0)])
        b.row(k % 3, mu, Lmod, pose_block(_unit(rng, (N,)) * rng.uniform(0, 1.3, (N, 1))), edge=False)
    return b.table(stream_offset=31)


P2_HEADINGS = (math.pi, -math.pi, 7.0)
P2_TRANSLATIONS = (1e-3, 1.0, 1e6)


def pose2_edge_table():
    """Pose2 edges, N = 34: fixed headings and measured headings at ±π exactly and at 7.0; θp + z_θ crossing ±π from both sides (σ_θ = 0.05
    around the cut, and 1e-9 either side of it); translations up to 1e6; each in dir 0, dir 1 and (the measured ones) as prior rows."""
    N = EDGE_N
    b = _Builder(P2P2, N, 6200)
    rng = b.rng

    def block(theta, tscale=3.0):
        return np.concatenate([rng.standard_normal((2, N)) * tscale, np.broadcast_to(np.asarray(theta, dtype=np.float64), (N,))[None]], 0)
    Lmod = _chol_rows(rng, 1, 3, [0.3, 0.3, 0.1])[0]
    for h in P2_HEADINGS:
        for dr in (0, 1):
            b.row(dr, rng.standard_normal(3) * [2, 2, 0.5], Lmod, block(h))
        for dr in (0, 1, DIR_PRIOR):
            b.row(dr, np.array([1.5, -0.5, h]), _diagL(3, [0.3, 0.3, 1e-9]), block(rng.uniform(-3, 3, N)))
    for thp in (3.0, -3.0):
        for off, sw in ((0.0, 0.05), (1e-9, 1e-12), (-1e-9, 1e-12)):
            zt = math.copysign(math.pi - 3.0, thp) + off                       # θp + z_θ = ±π + off
            b.row(0, np.array([1.0, 2.0, zt]), _diagL(3, [0.3, 0.3, sw]), block(thp))
            b.row(1, np.array([1.0, 2.0, -zt]), _diagL(3, [0.3, 0.3, sw]), block(thp))
    for s in P2_TRANSLATIONS:
        for dr in (0, 1, DIR_PRIOR):
            b.row(dr, rng.standard_normal(3) * [s, s, 0.5], _diagL(3, [0.1 * s, 0.1 * s, 0.05]), block(rng.uniform(-3, 3, N), tscale=s))
    for k in range(12):
        b.row(k % 3, rng.standard_normal(3) * [2, 2, 0.5], Lmod, block(rng.uniform(-3, 3, N)), edge=False)
    return b.table(stream_offset=41)


BR_RANGES = (1e-3, 1.0, 1e2, 1e4)


def br_edge_table():
    """bearing-range -> landmark edges, N = 34: θp + β crossing ±π from both sides, pose headings at ±π and 7.0, ρ from 1e-3 to 1e4 with
    μ_ρ = 8 σ_ρ exactly (|ξ| <= 6.7 for a 32-bit Box-Muller radius: no sampled range is negative), pose translations up to 1e6."""
    N = EDGE_N
    b = _Builder(BR0, N, 6300)
    rng = b.rng

    def block(theta, tscale=3.0):
        return np.concatenate([rng.standard_normal((2, N)) * tscale, np.broadcast_to(np.asarray(theta, dtype=np.float64), (N,))[None]], 0)
    for thp in (3.0, -3.0, math.pi, -math.pi, 7.0):
        for off, sb in ((0.0, 0.05), (1e-9, 1e-12), (-1e-9, 1e-12)):
            beta = math.copysign(math.pi, thp) - thp + off if abs(thp) < 4 else 0.3 + off
            b.row(0, np.array([beta, 5.0]), np.array([sb, 0.5]), block(thp))
    for rho in BR_RANGES:
        for ts in (1.0, 1e6):
            b.row(0, np.array([rng.uniform(-3, 3), rho]), np.array([0.05, rho / 8.0]), block(rng.uniform(-3, 3, N), tscale=ts))
    for k in range(8):
        b.row(0, np.array([rng.uniform(-3, 3), rng.uniform(2, 20)]), np.array([0.05, 0.2]), block(rng.uniform(-3, 3, N)), edge=False)
    t = b.table(stream_offset=51)
    t["rows4"][:, 3] = np.arange(t["n_conv"])[::-1]
    t["bel_target"] = np.random.default_rng(6301).standard_normal((t["n_conv"], 2, N)) * 5
    return t


EDGE_TABLES = {P2P2: pose2_edge_table, BR0: br_edge_table, P3P3: pose3_edge_table}


@functools.lru_cache(maxsize=None)
def shape_reference(kind, N):
    return Reference(shape_table(kind, N))


@functools.lru_cache(maxsize=None)
def edge_reference(kind):
    return Reference(EDGE_TABLES[kind]())


MIXED_N = 100


@functools.lru_cache(maxsize=None)
def mixed_reference(kind):
    """the table of the mixed-convergence tests (every row with a target variable of its own) and its reference, built once"""
    return Reference(shape_table(kind, MIXED_N, own_targets=True))


def mixed_start_mask(kind, mode, n_conv, N=MIXED_N):
    """(n_conv, N) bool: which particles start AT the root.  A thread of the packed sweep owns particles 2j, 2j + 1 and solves them one
    after the other, so a wave-wide ballot sees the FIRST particles of its 64 threads together, then the second ones.
    "parity": by the parity of the thread's pair index j -- both particles of a pair share a state, neighbouring lanes differ, so every
    ballot of every wave sees lanes at the root and lanes far from it.  "waves": whole wavefronts alternate (every ballot is uniform)."""
    if mode == "parity":
        return np.broadcast_to(((np.arange(N) // 2) % 2 == 0)[None, :], (n_conv, N)).copy()
    return wave_groups(kind, N, n_conv) % 2 == 0


def wave_groups(kind, N, n_conv):
    """(n_conv, N) -> the wavefront (0..3) of the packed block that owns each particle: thread = lc·H + i // 2, wave = thread >> 6"""
    s = launch_shape(N, n_conv)
    lc = (np.arange(n_conv) % s["CPB"])[:, None]
    return (lc * s["H"] + (np.arange(N) // 2)[None, :]) >> 6
