"""References for the parametric linearisation (rome_linearize: whitened residuals and Jacobians of the seven factor kinds).

Three independent sides, none of which is the kernel:
  * ref_rows      -- mpmath at DPS digits.  Residuals written from their definitions on group elements (rotation matrices, no expanded
                     forms), the SO(3) logarithm through atan2(‖skew part‖, trace part) (accurate at every angle below π), Jacobians by
                     central differences of that residual with step H along the documented retractions, angular entries differenced
                     UNWRAPPED (so a row on the ±π cut gets its true, smooth derivative), then left-multiplied by the row's W.
  * np_linearize  -- float64 NumPy, vectorised over rows: the residual formulas the reference project uses (Manifolds' exp / log forms,
                     sym_rem with its x ≈ π snap) and the closed-form Jacobians.  Serves every row of a table; checked against mp on a
                     subset (tests/test_lin_ref_host.py).
  * oracle_r      -- the C oracle's double residuals, whitened.

Step and precision: a bearing Jacobian at pose-landmark distance n has third derivatives of order 1/n³, so a central difference with
step h is off by (h/n)²/3 relative to the entry.  The smallest n in the tables is 1e-6 and the bounds go down to 64 ulp (1.4e-14):
h = 1e-20 leaves 3e-29 there, and at 50 digits the rounding part is 1e-50·1e6/1e-20 = 1e-24.

Tolerances (class Reference): per table and output, the deviation of the double-precision side from mp on the mp rows, per row
relative to max(1, largest |reference entry| of the row); the bound for the kernel is 8x that figure with a floor of 64 ulp, times the
row scale.  Nothing here comes from a GPU run.

The case tables of tests/test_gpu_linearize.py are built here as well, so that the CPU test can check that mp is finite on every row.
"""
import functools
import math

import mpmath as mpm
import numpy as np

PRIORPOSE2, POSE2POSE2, BEARINGRANGE, PRIORPOINT2, POSE3POSE3, PRIORPOSE3, BEARING = range(7)   # ROME_FACTOR_* of include/rome_mi355.h
KINDS = (PRIORPOSE2, POSE2POSE2, BEARINGRANGE, PRIORPOINT2, POSE3POSE3, PRIORPOSE3, BEARING)
NAMES = {PRIORPOSE2: "PriorPose2", POSE2POSE2: "Pose2Pose2", BEARINGRANGE: "Pose2Point2BearingRange", PRIORPOINT2: "PriorPoint2",
         POSE3POSE3: "Pose3Pose3", PRIORPOSE3: "PriorPose3", BEARING: "Pose2Point2Bearing"}
DIMS = {PRIORPOSE2: (3, 3, 3, 0), POSE2POSE2: (3, 3, 3, 3), BEARINGRANGE: (2, 2, 3, 2), PRIORPOINT2: (2, 2, 2, 0),
        POSE3POSE3: (6, 6, 6, 6), PRIORPOSE3: (6, 6, 6, 0), BEARING: (1, 1, 3, 2)}                  # dz, dr, da, db
ANGLE_ROW = {PRIORPOSE2: 2, POSE2POSE2: 2, BEARINGRANGE: 0, BEARING: 0}                            # the residual entry that lives on a circle
DPS = 50
H = "1e-20"
EPS = 2.0 ** -52
SQRT_EPS = 1.4901161193847656e-8


# =========================================================================================================== mpmath side
def _mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _mt(A):
    return [list(c) for c in zip(*A)]


def _mv(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def _rot2(th):
    c, s = mpm.cos(th), mpm.sin(th)
    return [[c, -s], [s, c]]


def _so3_exp(w):
    x, y, z = w
    th2 = x * x + y * y + z * z
    eye = [[mpm.mpf(i == j) for j in range(3)] for i in range(3)]
    if th2 == 0:
        return eye
    th = mpm.sqrt(th2)
    a = mpm.sin(th) / th
    hb = mpm.sin(th / 2) / th
    b = 2 * hb * hb                                           # (1 − cos θ)/θ² without the cancellation
    K = [[0, -z, y], [z, 0, -x], [-y, x, 0]]
    K2 = _mm(K, K)
    return [[eye[i][j] + a * K[i][j] + b * K2[i][j] for j in range(3)] for i in range(3)]


def _so3_log(R):
    """θ·axis with θ = atan2(‖vee(R − Rᵀ)/2‖, (tr R − 1)/2): no acos, no division by a vanishing sine below π"""
    v = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    s = mpm.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    c = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    if s == 0:
        if c < 0:
            raise ValueError("rotation by exactly π: the logarithm is not unique there")
        return [mpm.mpf(0)] * 3
    th = mpm.atan2(s, c)
    return [th / s * vi for vi in v]


def _point(dim, x):
    """coordinates (float64, taken exactly) -> group element: Point2 l, Pose2 (t, θ), Pose3 (t, R)"""
    x = [mpm.mpf(float(v)) for v in x]
    if dim == 2:
        return x
    if dim == 3:
        return (x[:2], x[2])
    return (x[:3], _so3_exp(x[3:]))


def _retract(dim, p, d):
    """the solver's retractions: Point2 l + δ ; Pose2 (t + δt, θ + δθ) ; Pose3 (t + δt, R·Exp(δω))"""
    if dim == 2:
        return [p[0] + d[0], p[1] + d[1]]
    if dim == 3:
        return ([p[0][0] + d[0], p[0][1] + d[1]], p[1] + d[2])
    return ([p[0][k] + d[k] for k in range(3)], _mm(p[1], _so3_exp(d[3:])))


def _angle2(U):
    return mpm.atan2(U[1][0], U[0][0])


def _bearing_range(pose, l):
    t, th = pose
    pl = _mv(_mt(_rot2(th)), [l[0] - t[0], l[1] - t[1]])
    return pl, mpm.atan2(pl[1], pl[0]), mpm.sqrt(pl[0] * pl[0] + pl[1] * pl[1])


def _wrap(x):
    return x - 2 * mpm.pi * mpm.nint(x / (2 * mpm.pi))


def _residual(kind, z, a, b):
    """z: the measurement coordinates (mpf list); a, b: group elements"""
    if kind == PRIORPOSE2:                                    # vee(log(p⁻¹ m)) on R² x SO(2)
        m = (z[:2], z[2])
        return [m[0][0] - a[0][0], m[0][1] - a[0][1], _angle2(_mm(_mt(_rot2(a[1])), _rot2(m[1])))]
    if kind == PRIORPOINT2:
        return [z[0] - a[0], z[1] - a[1]]
    if kind == POSE2POSE2:                                    # q̂ = p·Exp(z) = (p.t + Rp z_t, Rp Rz) ; vee(log(q⁻¹ q̂))
        Rp = _rot2(a[1])
        v = _mv(Rp, z[:2])
        U = _mm(_mt(_rot2(b[1])), _mm(Rp, _rot2(z[2])))
        return [a[0][0] + v[0] - b[0][0], a[0][1] + v[1] - b[0][1], _angle2(U)]
    if kind in (BEARINGRANGE, BEARING):
        _, ang, n = _bearing_range(a, b)
        r0 = _wrap(z[0] - ang)
        return [r0] if kind == BEARING else [r0, z[1] - n]
    if kind == POSE3POSE3:                                    # q̂ = (p.t + Rp z_t, Rp Exp(z_ω)) ; (q̂.t − q.t, log(Rqᵀ q̂.R))
        v = _mv(a[1], z[:3])
        U = _mm(_mt(b[1]), _mm(a[1], _so3_exp(z[3:])))
        return [a[0][k] + v[k] - b[0][k] for k in range(3)] + _so3_log(U)
    if kind == PRIORPOSE3:                                    # (m.t − p.t, log(Rpᵀ Rm))
        return [mpm.mpf(z[k]) - a[0][k] for k in range(3)] + _so3_log(_mm(_mt(a[1]), _so3_exp(z[3:])))
    raise NotImplementedError(kind)


def _jacobian(kind, z, a, b, which, r0):
    dz, dr, da, db = DIMS[kind]
    dim = da if which == 0 else db
    h = mpm.mpf(H)
    ang = ANGLE_ROW.get(kind, -1)
    J = [[None] * dim for _ in range(dr)]
    for j in range(dim):
        side = []
        for sgn in (1, -1):
            d = [mpm.mpf(0)] * dim
            d[j] = sgn * h
            rr = _residual(kind, z, _retract(dim, a, d), b) if which == 0 else _residual(kind, z, a, _retract(dim, b, d))
            side.append([_wrap(rr[i] - r0[i]) if i == ang else rr[i] - r0[i] for i in range(dr)])
        for i in range(dr):
            J[i][j] = (side[0][i] - side[1][i]) / (2 * h)
    return J


def _f64(M):
    return np.array([[float(v) for v in row] for row in M], dtype=np.float64)


def ref_rows(kind, mu, W, xa, xb, rows):
    """mp reference of the listed rows -> r (n, dr), Ja (n, dr, da), Jb (n, dr, db) or None, rounded to float64 at the very end"""
    dz, dr, da, db = DIMS[kind]
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, dz)
    W = np.asarray(W, dtype=np.float64).reshape(-1, dr, dr)
    xa = np.asarray(xa, dtype=np.float64).reshape(-1, da)
    xb = np.asarray(xb, dtype=np.float64).reshape(-1, db) if db else None
    n = len(rows)
    r = np.empty((n, dr))
    Ja = np.empty((n, dr, da))
    Jb = np.empty((n, dr, db)) if db else None
    with mpm.workdps(DPS):
        for k, f in enumerate(rows):
            z = [mpm.mpf(float(v)) for v in mu[f]]
            a = _point(da, xa[f])
            b = _point(db, xb[f]) if db else None
            Wf = [[mpm.mpf(float(v)) for v in row] for row in W[f]]
            r0 = _residual(kind, z, a, b)
            r[k] = [float(v) for v in _mv(Wf, r0)]
            Ja[k] = _f64(_mm(Wf, _jacobian(kind, z, a, b, 0, r0)))
            if db:
                Jb[k] = _f64(_mm(Wf, _jacobian(kind, z, a, b, 1, r0)))
    return r, Ja, Jb


def ref_residual(kind, mu, xa, xb, f):
    """the UNWHITENED mp residual of row f as floats (the tests use it to check where a constructed row really lies)"""
    dz, dr, da, db = DIMS[kind]
    with mpm.workdps(DPS):
        z = [mpm.mpf(float(v)) for v in np.asarray(mu)[f]]
        rr = _residual(kind, z, _point(da, np.asarray(xa)[f]), _point(db, np.asarray(xb)[f]) if db else None)
        return np.array([float(v) for v in rr])


def bearing_cut_distance(mu, xa, xb, f):
    """(b − atan2(pl)) − (±π) of a bearing row BEFORE wrapping, against the nearer of +π and −π -> (signed distance, which π)"""
    with mpm.workdps(DPS):
        _, ang, _ = _bearing_range(_point(3, np.asarray(xa)[f]), _point(2, np.asarray(xb)[f]))
        x = mpm.mpf(float(np.asarray(mu)[f][0])) - ang
        s = 1 if x > 0 else -1
        return float(x - s * mpm.pi), s


def pose3_compose(x, d):
    """coordinates of x ⊕ d = (t + d_t, Exp(ω)·Exp(d_ω)), the product formed in mp and rounded once (principal rotation vector)"""
    x = np.asarray(x, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    if not np.any(d[3:]):
        return np.concatenate([x[:3] + d[:3], x[3:]])
    with mpm.workdps(DPS):
        w = _so3_log(_mm(_so3_exp([mpm.mpf(float(v)) for v in x[3:]]), _so3_exp([mpm.mpf(float(v)) for v in d[3:]])))
        return np.concatenate([x[:3] + d[:3], [float(v) for v in w]])


# =========================================================================================================== float64 NumPy restatement
def _np_wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def _np_sym_rem(x):
    """Manifolds.sym_rem: x ≈ π (isapprox, rtol √eps) -> −π, else the IEEE remainder by 2π"""
    snap = np.abs(x - np.pi) <= SQRT_EPS * np.maximum(np.abs(x), np.pi)
    return np.where(snap, -np.pi, np.vectorize(math.remainder, otypes=[np.float64])(x, 2.0 * np.pi))


def _np_hat(w):
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1] = -w[..., 2]; K[..., 0, 2] = w[..., 1]
    K[..., 1, 0] = w[..., 2];  K[..., 1, 2] = -w[..., 0]
    K[..., 2, 0] = -w[..., 1]; K[..., 2, 1] = w[..., 0]
    return K


def _np_so3_exp(w):
    """Manifolds' exp!(::Rotations{3}): I + (sin θ/θ) K + ((1 − cos θ)/θ²) K²"""
    th2 = np.sum(w * w, axis=-1)
    th = np.sqrt(th2)
    nz = th != 0.0
    safe = np.where(nz, th, 1.0)
    a = np.where(nz, np.sin(safe) / safe, 1.0)[..., None, None]
    b = np.where(nz, (1.0 - np.cos(safe)) / (safe * safe), 0.0)[..., None, None]
    K = _np_hat(w)
    return np.eye(3) + a * K + b * (K @ K)


def _np_so3_log(U):
    """Manifolds' log!(::Rotations{3}), main branch: (U − Uᵀ)ᵛ / (2·sqrt(1 − c²)/acos c).  The cos θ ≈ −1 branch lies beyond π − 1e-3,
    where these tables stop; a row that would take it is an error, not a silent other formula."""
    c = 0.5 * (U[..., 0, 0] + U[..., 1, 1] + U[..., 2, 2] - 1.0)
    if np.any(np.abs(c + 1.0) <= SQRT_EPS):
        raise ValueError("residual rotation within sqrt(eps) of π")
    s = np.stack([U[..., 2, 1] - U[..., 1, 2], U[..., 0, 2] - U[..., 2, 0], U[..., 1, 0] - U[..., 0, 1]], axis=-1)
    inner = (c < 1.0) & (c > -1.0)
    cc = np.where(inner, c, 0.0)
    usinc = np.where(c >= 1.0, 1.0, np.where(inner, np.sqrt(1.0 - cc * cc) / np.arccos(cc), 0.0))
    return (0.5 / usinc)[..., None] * s


def _np_jinv(phi, sign):
    """J_r⁻¹ (sign +1) / J_l⁻¹ (sign −1) of SO(3): I ± ½[φ]× + c[φ]×², c = 1/θ² − (1 + cos θ)/(2θ sin θ); below θ = 1e-2 the series
    1/12 + θ²/720 + θ⁴/30240 (next term θ⁶/1209600 < 1e-18 there; the closed form's cancellation is eps/θ² <= 2e-12 above)"""
    th2 = np.sum(phi * phi, axis=-1)
    small = th2 < 1e-4
    th = np.sqrt(np.where(small, 1.0, th2))
    c = np.where(small, 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0,
                 1.0 / np.where(small, 1.0, th2) - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th)))
    K = _np_hat(phi)
    return np.eye(3) + 0.5 * sign * K + c[..., None, None] * (K @ K)


def np_rows(kind, mu, xa, xb=None):
    """unwhitened residual and Jacobians of every row, float64 -> rr (F, dr), JA (F, dr, da), JB (F, dr, db) or None"""
    dz, dr, da, db = DIMS[kind]
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, dz)
    xa = np.asarray(xa, dtype=np.float64).reshape(-1, da)
    xb = np.asarray(xb, dtype=np.float64).reshape(-1, db) if db else None
    F = len(mu)
    JB = None
    if kind == PRIORPOSE2:
        rr = np.stack([mu[:, 0] - xa[:, 0], mu[:, 1] - xa[:, 1], _np_wrap(mu[:, 2] - xa[:, 2])], 1)
        JA = np.tile(-np.eye(3), (F, 1, 1))
    elif kind == PRIORPOINT2:
        rr = mu - xa
        JA = np.tile(-np.eye(2), (F, 1, 1))
    elif kind == POSE2POSE2:
        c, s = np.cos(xa[:, 2]), np.sin(xa[:, 2])
        rr = np.stack([xa[:, 0] + c * mu[:, 0] - s * mu[:, 1] - xb[:, 0], xa[:, 1] + s * mu[:, 0] + c * mu[:, 1] - xb[:, 1],
                       _np_wrap(xa[:, 2] + mu[:, 2] - xb[:, 2])], 1)
        JA = np.tile(np.eye(3), (F, 1, 1)); JA[:, 0, 2] = -s * mu[:, 0] - c * mu[:, 1]; JA[:, 1, 2] = c * mu[:, 0] - s * mu[:, 1]
        JB = np.tile(-np.eye(3), (F, 1, 1))
    elif kind in (BEARINGRANGE, BEARING):
        c, s = np.cos(xa[:, 2]), np.sin(xa[:, 2])
        dx, dy = xb[:, 0] - xa[:, 0], xb[:, 1] - xa[:, 1]
        plx, ply = c * dx + s * dy, c * dy - s * dx
        with np.errstate(divide="ignore", invalid="ignore"):
            n2 = plx * plx + ply * ply
            n = np.sqrt(n2)
            A = np.empty((F, 2, 2))                           # ∂(bearing residual, range residual)/∂pl
            A[:, 0, 0] = ply / n2; A[:, 0, 1] = -plx / n2; A[:, 1, 0] = -plx / n; A[:, 1, 1] = -ply / n
            Rt = np.empty((F, 2, 2)); Rt[:, 0, 0] = c; Rt[:, 0, 1] = s; Rt[:, 1, 0] = -s; Rt[:, 1, 1] = c     # ∂pl/∂l = Rᵀ = −∂pl/∂t
            JB = A @ Rt
        JA = np.concatenate([-JB, np.tile(np.array([[1.0], [0.0]]), (F, 1, 1))], axis=2)   # ∂pl/∂θ = (pl_y, −pl_x): A·that = (1, 0)
        rr = np.stack([_np_sym_rem(mu[:, 0] - np.arctan2(ply, plx)), (mu[:, 1] if kind == BEARINGRANGE else 0.0) - n], 1)
        if kind == BEARING:
            rr, JA, JB = rr[:, :1], JA[:, :1], JB[:, :1]
    elif kind == POSE3POSE3:
        Rp, Rq, Z = _np_so3_exp(xa[:, 3:]), _np_so3_exp(xb[:, 3:]), _np_so3_exp(mu[:, 3:])
        rw = _np_so3_log(np.swapaxes(Rq, 1, 2) @ (Rp @ Z))
        rr = np.concatenate([xa[:, :3] + np.einsum("fij,fj->fi", Rp, mu[:, :3]) - xb[:, :3], rw], 1)
        JA = np.zeros((F, 6, 6)); JB = np.zeros((F, 6, 6))
        JA[:, :3, :3] = np.eye(3); JB[:, :3, :3] = -np.eye(3)
        JA[:, :3, 3:] = -Rp @ _np_hat(mu[:, :3])              # ∂(Rp Exp(δ) z_t)/∂δ
        JA[:, 3:, 3:] = _np_jinv(rw, +1.0) @ np.swapaxes(Z, 1, 2)
        JB[:, 3:, 3:] = -_np_jinv(rw, -1.0)
    elif kind == PRIORPOSE3:
        Rp, Rm = _np_so3_exp(xa[:, 3:]), _np_so3_exp(mu[:, 3:])
        rw = _np_so3_log(np.swapaxes(Rp, 1, 2) @ Rm)
        rr = np.concatenate([mu[:, :3] - xa[:, :3], rw], 1)
        JA = np.zeros((F, 6, 6)); JA[:, :3, :3] = -np.eye(3); JA[:, 3:, 3:] = -_np_jinv(rw, -1.0)
    else:
        raise NotImplementedError(kind)
    return rr, JA, JB


def np_linearize(kind, mu, W, xa, xb=None, ctx=None):
    """float64 stand-in with the signature of rome_jl_amd.linearize: whitened residuals and Jacobians of all seven kinds"""
    rr, JA, JB = np_rows(kind, mu, xa, xb)
    W = np.asarray(W, dtype=np.float64).reshape(len(rr), rr.shape[1], rr.shape[1])
    return np.einsum("fij,fj->fi", W, rr), W @ JA, (None if JB is None else W @ JB)


def oracle_r(kind, mu, W, xa, xb=None):
    """the C oracle's double residuals, whitened"""
    import oracle as ro
    mu = np.ascontiguousarray(mu, dtype=np.float64); xa = np.ascontiguousarray(xa, dtype=np.float64)
    xb = None if xb is None else np.ascontiguousarray(xb, dtype=np.float64)
    if kind == PRIORPOSE2: rr = ro.residual_priorpose2(mu, xa)
    elif kind == POSE2POSE2: rr = ro.residual_pose2pose2(mu, xa, xb)
    elif kind == BEARINGRANGE: rr = ro.residual_pose2point2br(mu, xa, xb)
    elif kind == BEARING: rr = ro.residual_pose2point2br(np.concatenate([mu, np.zeros_like(mu)], 1), xa, xb)[:, :1]
    elif kind == PRIORPOINT2: rr = mu - xa
    elif kind == POSE3POSE3: rr = ro.residual_pose3pose3(mu, xa, xb)
    else: rr = ro.residual_priorpose3(mu, xa)
    return np.einsum("fij,fj->fi", np.asarray(W, dtype=np.float64), np.asarray(rr).reshape(len(mu), -1))


# =========================================================================================================== deviations and bounds
def row_scale(ref):
    """max(1, largest |reference entry| of the row), one value per row"""
    ref = np.asarray(ref)
    return np.maximum(1.0, np.abs(ref.reshape(len(ref), -1)).max(axis=1))


def deviation(kind, W, got, ref, wrapped=False):
    """per-row max |got − ref|.  wrapped: the residual's circle entry may differ by a whole turn, which shows in the whitened vector
    as ±2π times that column of W; the smallest of the three candidates counts."""
    got = np.asarray(got); ref = np.asarray(ref)
    n = len(ref)
    d = np.abs((got - ref).reshape(n, -1)).max(axis=1)
    if wrapped and kind in ANGLE_ROW:
        col = np.asarray(W)[:, :, ANGLE_ROW[kind]]
        for k in (-1.0, 1.0):
            d = np.minimum(d, np.abs(got - ref - k * 2.0 * np.pi * col).reshape(n, -1).max(axis=1))
    return d


def subset_rows(F, seed=0):
    """the rows the mp reference serves in a table of F rows: the block edges plus 8 seeded random rows"""
    fixed = [0, 1, 62, 63, 64, 65, F - 2, F - 1]
    rnd = np.random.default_rng(1000 + seed).integers(0, F, 8).tolist()
    return sorted({f for f in fixed + rnd if 0 <= f < F})


class Reference:
    """Everything a test needs about one table, computed once: the mp rows, the NumPy restatement and the oracle residual of all rows,
    the reference-side error figures and the bounds derived from them."""

    def __init__(self, table, rows=None):
        kind = self.kind = table["kind"]
        self.table = table
        mu, W, xa, xb = table["mu"], table["W"], table["xa"], table.get("xb")
        F = self.F = len(mu)
        skip = table.get("excluded")
        self.rows = [f for f in (list(range(F)) if rows is None else rows) if f != skip]
        self.mp = dict(zip(("r", "Ja", "Jb"), ref_rows(kind, mu, W, xa, xb, self.rows)))
        with np.errstate(all="ignore"):
            self.np = dict(zip(("r", "Ja", "Jb"), np_linearize(kind, mu, W, xa, xb)))
            self.oracle = oracle_r(kind, mu, W, xa, xb)
        self.outputs = ("r", "Ja", "Jb") if DIMS[kind][3] else ("r", "Ja")
        self.scale = {o: row_scale(self.mp[o]) for o in self.outputs}
        Wm = np.asarray(W)[self.rows]
        self.dev = {"r": deviation(kind, Wm, self.oracle[self.rows], self.mp["r"], wrapped=True) / self.scale["r"],
                    "r_np": deviation(kind, Wm, self.np["r"][self.rows], self.mp["r"], wrapped=True) / self.scale["r"]}
        for o in self.outputs[1:]:
            self.dev[o] = deviation(kind, Wm, self.np[o][self.rows], self.mp[o]) / self.scale[o]
        self.figure = {o: float(self.dev[o].max()) for o in self.outputs}
        self.rel_bound = {o: max(8.0 * self.figure[o], 64.0 * EPS) for o in self.outputs}

    def check_mp(self, out, got):
        """kernel output `got` (all F rows) against mp on the mp rows -> (largest deviation / row scale, the bound it must not exceed)"""
        d = deviation(self.kind, np.asarray(self.table["W"])[self.rows], np.asarray(got)[self.rows], self.mp[out], wrapped=(out == "r"))
        return float((d / self.scale[out]).max()), self.rel_bound[out]

    def check_np(self, out, got, upto=None):
        """kernel output against the double-precision side (the oracle for r, the NumPy restatement for the Jacobians) on rows
        [0, upto), the excluded row left out -> (worst deviation / row scale, bound)"""
        n = self.F if upto is None else upto
        keep = [f for f in range(n) if f != self.table.get("excluded")]
        ref = (self.oracle if out == "r" else self.np[out])[keep]
        d = deviation(self.kind, np.asarray(self.table["W"])[keep], np.asarray(got)[keep], ref, wrapped=(out == "r"))
        return float((d / row_scale(ref)).max()), self.rel_bound[out]


# =========================================================================================================== case tables
def dense_W(rng, F, dr):
    """a distinct, dense, non-symmetric whitening matrix per row"""
    return np.eye(dr) + 0.3 * rng.standard_normal((F, dr, dr))


def _rotvec(rng, F, scale):
    return rng.standard_normal((F, 3)) * scale


def _br_landmark(pose, n, beta):
    """the landmark at distance n and body-frame bearing beta of the pose"""
    return np.array([pose[0] + n * math.cos(pose[2] + beta), pose[1] + n * math.sin(pose[2] + beta)])


def geometry_table(kind, F=129, seed=0):
    """one seeded table of ordinary rows per kind; the second variable is the first composed with the measurement plus noise, so that
    the residuals are moderate (no rotation near π by accident)"""
    rng = np.random.default_rng(4200 + 10 * kind + seed)
    dz, dr, da, db = DIMS[kind]
    t = {"kind": kind, "W": dense_W(rng, F, dr), "xb": None}
    if kind in (PRIORPOSE2, POSE2POSE2):
        t["mu"] = rng.standard_normal((F, 3)) * [3, 3, 1.5]
        t["xa"] = rng.standard_normal((F, 3)) * [8, 8, 3]
        if kind == PRIORPOSE2:
            t["xa"] = t["mu"] + rng.standard_normal((F, 3)) * [1, 1, 0.8]
        else:
            t["xb"] = rng.standard_normal((F, 3)) * [8, 8, 3]
    elif kind == PRIORPOINT2:
        t["mu"] = rng.standard_normal((F, 2)) * 5
        t["xa"] = rng.standard_normal((F, 2)) * 5
    elif kind in (BEARINGRANGE, BEARING):
        t["xa"] = rng.standard_normal((F, 3)) * [8, 8, 3]
        n = rng.uniform(0.5, 20, F)
        beta = rng.uniform(-3.1, 3.1, F)
        t["xb"] = np.stack([_br_landmark(t["xa"][f], n[f], beta[f]) for f in range(F)])
        b = beta + rng.uniform(-2.5, 2.5, F)                                   # residual in (−2.5, 2.5): the cut rows are built on purpose elsewhere
        t["mu"] = np.stack([b, n + rng.standard_normal(F)], 1) if kind == BEARINGRANGE else b[:, None]
    else:
        t["mu"] = np.concatenate([rng.standard_normal((F, 3)) * 2, _rotvec(rng, F, 0.5)], 1)
        t["xa"] = np.concatenate([rng.standard_normal((F, 3)) * 5, _rotvec(rng, F, 0.7)], 1)
        noise = np.concatenate([rng.standard_normal((F, 3)), _rotvec(rng, F, 0.4)], 1)
        if kind == PRIORPOSE3:
            t["xa"] = np.stack([pose3_compose(t["mu"][f], noise[f]) for f in range(F)])
        else:
            t["xb"] = np.stack([pose3_compose(pose3_compose(t["xa"][f], t["mu"][f]), noise[f]) for f in range(F)])
            t["xb"][:, :3] = t["xa"][:, :3] + rng.standard_normal((F, 3)) * 3
    return t


HEADINGS = (math.pi, -math.pi, math.pi - 1e-12, -(math.pi - 1e-12), 3 * math.pi, -7.5, 1e3)
DISTANCES = (1e-6, 1e-3, 1.0, 1e3, 1e6)
ORIGINS = ((0.3, -0.2), (1e6, -1e6))
CUT_OFFSETS = (1e-9, 1e-4)


def _stack(kind, rows, seed):
    """rows: list of (mu, xa, xb) -> a table with a dense W per row"""
    dz, dr, da, db = DIMS[kind]
    rng = np.random.default_rng(seed)
    return {"kind": kind, "mu": np.array([np.atleast_1d(r[0]) for r in rows], dtype=np.float64).reshape(-1, dz),
            "W": dense_W(rng, len(rows), dr), "xa": np.array([r[1] for r in rows], dtype=np.float64),
            "xb": np.array([r[2] for r in rows], dtype=np.float64) if db else None}


def _bearing_row(kind, pose, n, b, resid):
    """measured bearing b (and a measured range of 1.5 n), the landmark at distance n where the bearing residual is `resid`"""
    l = _br_landmark(pose, n, b - resid)
    return ([b, 1.5 * n] if kind == BEARINGRANGE else [b]), np.array(pose, dtype=np.float64), l


def pose2_edge_tables(kind):
    """group name -> table, for PriorPose2, Pose2Pose2, bearing-range and bearing-only"""
    rng = np.random.default_rng(7700 + kind)
    g = {}
    if kind in (PRIORPOSE2, POSE2POSE2):
        rows = []
        for h in HEADINGS:                                                    # the extreme heading in each argument in turn
            for slot in range(3 if kind == POSE2POSE2 else 2):
                mu = rng.standard_normal(3) * [3, 3, 1.0]
                xa = rng.standard_normal(3) * [8, 8, 1.0]
                xb = rng.standard_normal(3) * [8, 8, 1.0]
                (mu, xa, xb)[slot][2] = h
                rows.append((mu, xa, xb))
        g["headings"] = _stack(kind, rows, 7710 + kind)
        rows = []
        for sgn in (1.0, -1.0):                                               # heading residual within 1e-12 of ±π, on either side
            for off in (1e-12, -1e-12):
                tha, thz = 0.7, 1.1
                target = sgn * (math.pi - off)
                if kind == POSE2POSE2:
                    rows.append(([1.5, -0.5, thz], [2.0, 1.0, tha], [3.0, 0.5, tha + thz - target]))
                else:
                    rows.append(([1.5, -0.5, thz], [2.0, 1.0, thz - target], None))
        g["cut"] = _stack(kind, rows, 7720 + kind)
    else:
        rows = [_bearing_row(kind, [1.0, -2.0, h], 3.0, 0.4, 0.3) for h in HEADINGS]
        rows += [_bearing_row(kind, [1.0, -2.0, 0.6], 3.0, h, 0.3) for h in HEADINGS if abs(h) < 100.0]
        g["headings"] = _stack(kind, rows, 7710 + kind)
        # a MEASURED bearing of 1e3 enters b − atan2(pl), which rounds at ulp(1e3)/2: a group of its own, so that the other
        # headings keep the 64 ulp floor
        g["bearing_1e3"] = _stack(kind, [_bearing_row(kind, [1.0, -2.0, 0.6], 3.0, h, 0.3) for h in HEADINGS if abs(h) >= 100.0], 7750 + kind)
        cut, snap = [], []
        for off in CUT_OFFSETS:                                               # x = b − atan2(pl) on both sides of +π and of −π
            for b, x in ((2.0, math.pi - off), (2.0, math.pi + off), (-2.0, -math.pi + off), (-2.0, -math.pi - off)):
                row = _bearing_row(kind, [0.5, -0.25, 0.6], 2.5, b, x)
                (snap if (x > 0 and off < 1e-8) else cut).append(row)          # sym_rem snaps |x − π| <= √eps·π to −π exactly
        g["cut"] = _stack(kind, cut, 7720 + kind)
        g["cut_snap"] = _stack(kind, snap, 7730 + kind)
        g["distance"] = _stack(kind, [_bearing_row(kind, [o[0], o[1], 0.9], n, 0.4, 0.3) for o in ORIGINS for n in DISTANCES], 7740 + kind)
    return g


def n2zero_tables(kind):
    """a 129-row bearing table with the landmark of row 70 exactly on its pose, and the same table with an ordinary row there"""
    t = geometry_table(kind, 129, seed=5)
    bad = {k: (v if v is None or k == "kind" else np.array(v, copy=True)) for k, v in t.items()}
    bad["xb"][70] = bad["xa"][70, :2]
    bad["excluded"] = 70
    return bad, t


# residual rotations |φ| by group: each group gets its own reference-error figure, because the error of the shared log formula
# sqrt(1 − c²)/acos(c) depends on the angle (rounding of c² near c = ±1) and must not widen the bound of the other rows
PHI_GROUPS = {"phi_tiny": (0.0, 1e-12, 1e-6),
              "phi_switch": (0.99e-4, 1.01e-4, 1e-3),                           # 0.99e-4 | 1.01e-4: the two sides of so3_jinv's series switch
              "phi_mid": (0.1, 1.0, 2.0, 3.0),
              "near_pi_1e-2": (math.pi - 1e-2,), "near_pi_1e-3": (math.pi - 1e-3,)}
POSE_NORMS = (0.0, 1e-9, math.pi - 1e-6, 4.0, 7.0)
AXES = (np.array([0.36, -0.48, 0.8]), np.array([0.0, 1.0, 0.0]),                # generic unit axes and coordinate axes: the error of the
        np.array([-0.6, 0.64, 0.48]), np.array([0.0, 0.0, -1.0]))              # shared log formula is a rounding, so more than one sample each
# The figure of phi_switch, phi_mid and near_pi_* is the largest of these four roundings, and the kernel's bound is 8x it: that margin
# is statistical, not a worst case.  The kernel rounds the same formula in another order and has been seen at 2x the figure; another
# libm or seed can move the figure by a similar factor.  The worst case of the formula is log_formula_error below, which the CPU test
# holds the figure under; it lies 3x to 80x above the figures, so the sampled figure is the tighter bound and is the one used.


def log_formula_error(theta):
    """What sqrt(1 − c²)/acos(c) can lose at residual angle θ, as an absolute error of the rotation vector: c carries about eps from
    the trace of a rounded matrix product and c² rounds at eps/2, so 1 − c² = sin²θ is off by about eps, the ratio by eps/(2 sin²θ)
    relative, and the vector of length θ by eps·θ/(2 sin²θ).  A dense whitening row (|W| row sums up to about 3) and so3_jinv, which
    is evaluated at that vector, carry it into every output: 4·eps·θ/sin²θ in all, relative to a row scale of at least 1."""
    return 4.0 * EPS * theta / math.sin(theta) ** 2


def pose3_edge_tables(kind):
    """group name -> table for Pose3Pose3 and PriorPose3.  In the PHI_GROUPS the rows of one axis share everything but |φ| (also
    the W), so that two neighbouring rows differ by the residual rotation alone."""
    rng = np.random.default_rng(8800 + kind)
    g = {}

    def sweep(norms, seed):
        rows, Ws = [], []
        for ax in AXES:
            base = np.concatenate([rng.standard_normal(3) * 4, _rotvec(rng, 1, 0.6)[0]])
            zt = rng.standard_normal(3) * 2
            dt = rng.standard_normal(3)
            W = dense_W(rng, 1, 6)[0]
            for nrm in norms:
                d = np.concatenate([dt, nrm * ax])
                if kind == POSE3POSE3:                                          # z_ω = 0, xb = xa ⊕ (δt, φ): residual rotation −φ
                    rows.append((np.concatenate([zt, np.zeros(3)]), base, pose3_compose(base, d)))
                else:                                                           # xa = μ ⊕ (δt, φ)
                    rows.append((base, pose3_compose(base, d), None))
                Ws.append(W)
        t = _stack(kind, rows, seed)
        t["W"] = np.array(Ws)
        return t
    for i, (name, norms) in enumerate(PHI_GROUPS.items()):
        g[name] = sweep(norms, 8810 + 10 * i + kind)
    rows = []
    gen = AXES[0]
    for nrm in POSE_NORMS:                                                      # pose coordinates at the zero guard and beyond the principal range
        far = np.concatenate([rng.standard_normal(3) * 4, nrm * gen])
        d = np.concatenate([rng.standard_normal(3), 0.4 * np.array([0.6, 0.0, -0.8])])
        zt = np.concatenate([rng.standard_normal(3) * 2, np.zeros(3)])
        if kind == POSE3POSE3:
            rows.append((zt, far, pose3_compose(far, d)))                       # the extreme vector as xa ...
            rows.append((zt, pose3_compose(far, d), far))                       # ... and as xb
        else:
            rows.append((pose3_compose(far, d), far, None))
            rows.append((far, pose3_compose(far, d), None))
    g["pose_coords"] = _stack(kind, rows, 8930 + kind)
    rows = []
    for nrm in (0.0, 3.0):                                                      # measurement rotations of 0 and 3 with translations of 1e3
        for ax in AXES:
            z = np.concatenate([rng.standard_normal(3) * 1e3, nrm * ax])
            d = np.concatenate([rng.standard_normal(3), 0.3 * np.array([0.0, 0.6, 0.8])])
            if kind == POSE3POSE3:
                xa = np.concatenate([rng.standard_normal(3) * 1e3, _rotvec(rng, 1, 0.6)[0]])
                xb = pose3_compose(pose3_compose(xa, np.concatenate([np.zeros(3), z[3:]])), d)
                xb[:3] = xa[:3] + rng.standard_normal(3) * 1e3
                rows.append((z, xa, xb))
            else:
                rows.append((z, pose3_compose(z, d), None))
    g["meas_rot"] = _stack(kind, rows, 8940 + kind)
    return g


POSE2_EDGE_KINDS = (PRIORPOSE2, POSE2POSE2, BEARINGRANGE, BEARING)
POSE3_EDGE_KINDS = (POSE3POSE3, PRIORPOSE3)


@functools.lru_cache(maxsize=None)
def geometry_reference(kind):
    t = geometry_table(kind)
    return Reference(t, subset_rows(len(t["mu"]), kind))


@functools.lru_cache(maxsize=None)
def edge_references(kind):
    """group name -> Reference with every row served by mp"""
    tables = pose2_edge_tables(kind) if kind in POSE2_EDGE_KINDS else pose3_edge_tables(kind)
    return {name: Reference(t) for name, t in tables.items()}
