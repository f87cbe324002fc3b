"""References for the deconvolution (rome_deconv*, k_deconv): the measurement a pair of particles predicts for a relative factor.

Two sides that share nothing with the kernel (in the manner of lin_ref.py):
  * mp_predict   -- mpmath at 50 digits, written from the definitions on group elements: rotations as matrices (Rodrigues from the
                    rotation vector), the SO(3) logarithm through atan2(|skew part|, trace part), headings through atan2 of the
                    relative rotation's first column;
  * np_predict   -- the same definitions in float64 NumPy over whole tables (3x3 matrices; the kernel works on unit quaternions and
                    on (cos, sin) pairs).

Bounds (class Reference; this project's standing rule, lin_ref.Reference): per family, the deviation of the float64 side from mp on
the mp rows, per row relative to max(1, largest |reference entry| of the row); the bound for the kernel is 8x that figure with a floor
of 64 ulp, times the same row scale.  Computed on the CPU, never from a GPU run.  Angular entries are compared modulo 2 pi.
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = float(np.finfo(np.float64).eps)

# family -> (factor class name, dz, dimension of the first / second variable, angular entries of the measurement)
FAMILIES = {
    "p2p2": ("Pose2Pose2", 3, 3, 3, (2,)),
    "br": ("Pose2Point2BearingRange", 2, 3, 2, (0,)),
    "pbear": ("Pose2Point2Bearing", 1, 3, 2, (0,)),
    "p2rng": ("Point2Point2Range", 1, 2, 2, ()),
    "pprng": ("Pose2Point2Range", 1, 3, 2, ()),
    "p3p3": ("Pose3Pose3", 6, 6, 6, ()),
    "p3xyy": ("Pose3Pose3XYYaw", 3, 6, 6, (2,)),
    "p3rot": ("Pose3Pose3Rotation", 3, 6, 6, ()),
}


# =========================================================================================================== mpmath
def _mp_so3_exp(w):
    w = [mp.mpf(float(x)) for x in w]
    th = mp.sqrt(sum(x * x for x in w))
    K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)


def _mp_so3_log(U):
    v = [U[2, 1] - U[1, 2], U[0, 2] - U[2, 0], U[1, 0] - U[0, 1]]
    s = mp.sqrt(sum(x * x for x in v)) / 2
    c = (U[0, 0] + U[1, 1] + U[2, 2] - 1) / 2
    if s == 0:
        return [mp.mpf(0)] * 3
    th = mp.atan2(s, c)
    return [th * x / (2 * s) for x in v]


def _mp_se2(p, q):
    """(R_p^T (t_q - t_p), angle of R_p^T R_q) from (x, y, cos, sin) of both"""
    dx, dy = q[0] - p[0], q[1] - p[1]
    return [p[2] * dx + p[3] * dy, p[2] * dy - p[3] * dx, mp.atan2(p[2] * q[3] - p[3] * q[2], p[2] * q[2] + p[3] * q[3])]


def _mp_pose2(x):
    x = [mp.mpf(float(v)) for v in x]
    return [x[0], x[1], mp.cos(x[2]), mp.sin(x[2])]


def _mp_proj(x):
    """the SE(2) projection of Pose3 coordinates: t_xy and the normalised first column of R"""
    R = _mp_so3_exp(x[3:6])
    n = mp.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2)
    return [mp.mpf(float(x[0])), mp.mpf(float(x[1])), R[0, 0] / n, R[1, 0] / n]


def mp_predict(family, a, b):
    """one row at 50 digits -> list of dz mpf"""
    if family == "p2p2":
        return _mp_se2(_mp_pose2(a), _mp_pose2(b))
    if family in ("br", "pbear"):
        p = _mp_pose2(a)
        dx, dy = mp.mpf(float(b[0])) - p[0], mp.mpf(float(b[1])) - p[1]
        plx, ply = p[2] * dx + p[3] * dy, p[2] * dy - p[3] * dx
        bearing = mp.atan2(ply, plx)
        return [bearing] if family == "pbear" else [bearing, mp.sqrt(plx * plx + ply * ply)]
    if family in ("p2rng", "pprng"):
        dx, dy = mp.mpf(float(b[0])) - mp.mpf(float(a[0])), mp.mpf(float(b[1])) - mp.mpf(float(a[1]))
        return [mp.sqrt(dx * dx + dy * dy)]
    if family == "p3xyy":
        return _mp_se2(_mp_proj(a), _mp_proj(b))
    Rp, Rq = _mp_so3_exp(a[3:6]), _mp_so3_exp(b[3:6])
    w = _mp_so3_log(Rp.T * Rq)
    if family == "p3rot":
        return w
    d = mp.matrix([mp.mpf(float(b[k])) - mp.mpf(float(a[k])) for k in range(3)])
    t = Rp.T * d
    return [t[0], t[1], t[2]] + w


# =========================================================================================================== float64 NumPy
def _np_so3_exp(w):
    w = np.asarray(w, dtype=np.float64)
    th2 = (w * w).sum(-1)
    th = np.sqrt(th2)
    safe = np.where(th > 0, th, 1.0)
    a = np.where(th > 0, np.sin(safe) / safe, 1.0)
    b = np.where(th > 0, (1.0 - np.cos(safe)) / (safe * safe), 0.5)
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def _np_so3_log(U):
    v = np.stack([U[..., 2, 1] - U[..., 1, 2], U[..., 0, 2] - U[..., 2, 0], U[..., 1, 0] - U[..., 0, 1]], axis=-1)
    s = 0.5 * np.sqrt((v * v).sum(-1))
    c = 0.5 * (np.trace(U, axis1=-2, axis2=-1) - 1.0)
    th = np.arctan2(s, c)
    k = np.where(s > 0, th / np.where(s > 0, 2.0 * s, 1.0), 0.5)
    return k[..., None] * v


def _np_se2(px, py, pc, ps, qx, qy, qc, qs):
    dx, dy = qx - px, qy - py
    return np.stack([pc * dx + ps * dy, pc * dy - ps * dx, np.arctan2(pc * qs - ps * qc, pc * qc + ps * qs)], axis=-1)


def _np_proj(x):
    R = _np_so3_exp(x[:, 3:6])
    n = np.hypot(R[:, 0, 0], R[:, 1, 0])
    return x[:, 0], x[:, 1], R[:, 0, 0] / n, R[:, 1, 0] / n


def np_predict(family, A, B):
    """F rows of first / second variable coordinates -> (F, dz) float64"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if family == "p2p2":
        return _np_se2(A[:, 0], A[:, 1], np.cos(A[:, 2]), np.sin(A[:, 2]), B[:, 0], B[:, 1], np.cos(B[:, 2]), np.sin(B[:, 2]))
    if family in ("br", "pbear"):
        c, s = np.cos(A[:, 2]), np.sin(A[:, 2])
        dx, dy = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1]
        plx, ply = c * dx + s * dy, c * dy - s * dx
        bearing = np.arctan2(ply, plx)
        return bearing[:, None] if family == "pbear" else np.stack([bearing, np.hypot(plx, ply)], axis=-1)
    if family in ("p2rng", "pprng"):
        return np.hypot(B[:, 0] - A[:, 0], B[:, 1] - A[:, 1])[:, None]
    if family == "p3xyy":
        return _np_se2(*_np_proj(A), *_np_proj(B))
    Rp, Rq = _np_so3_exp(A[:, 3:6]), _np_so3_exp(B[:, 3:6])
    RpT = np.swapaxes(Rp, -1, -2)
    w = _np_so3_log(RpT @ Rq)
    if family == "p3rot":
        return w
    t = (RpT @ (B[:, :3] - A[:, :3])[..., None])[..., 0]
    return np.concatenate([t, w], axis=-1)


# =========================================================================================================== deviations and bounds
def row_scale(ref):
    ref = np.asarray(ref, dtype=np.float64)
    return np.maximum(1.0, np.abs(ref.reshape(len(ref), -1)).max(axis=1))


def deviation(family, got, ref):
    """per-row max |got - ref|, the angular entries modulo 2 pi"""
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    for k in FAMILIES[family][4]:
        d[:, k] = np.arctan2(np.sin(d[:, k]), np.cos(d[:, k]))
    return np.abs(d).max(axis=1)


def subset_rows(F, seed=0):
    """the rows the mp reference serves in a table of F rows: the block edges plus 8 seeded random rows"""
    fixed = [0, 1, 62, 63, 64, 65, F - 2, F - 1]
    rnd = np.random.default_rng(1000 + seed).integers(0, F, 8).tolist()
    return sorted({f for f in fixed + rnd if 0 <= f < F})


class Reference:
    """One table of pairs (A, B): the mp rows, the NumPy restatement of all rows, the CPU-side figure and the bound derived from it."""

    def __init__(self, family, A, B, rows=None):
        self.family, self.A, self.B = family, np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        F = self.F = len(self.A)
        self.rows = list(range(F)) if rows is None else list(rows)
        self.mp_raw = [mp_predict(family, self.A[f], self.B[f]) for f in self.rows]
        self.mp = np.array([[float(x) for x in r] for r in self.mp_raw], dtype=np.float64).reshape(len(self.rows), -1)
        with np.errstate(all="ignore"):
            self.np = np_predict(family, self.A, self.B)
        self.scale = row_scale(self.mp)
        self.dev = deviation(family, self.np[self.rows], self.mp) / self.scale
        self.figure = float(self.dev.max())
        self.rel_bound = max(8.0 * self.figure, 64.0 * EPS)

    def check_mp(self, got):
        """kernel output (F, dz) against mp on the mp rows -> (largest deviation / row scale, bound)"""
        return float((deviation(self.family, np.asarray(got)[self.rows], self.mp) / self.scale).max()), self.rel_bound

    def check_np(self, got):
        """kernel output against the NumPy restatement on all rows -> (largest deviation / row scale, bound)"""
        return float((deviation(self.family, got, self.np) / row_scale(self.np)).max()), self.rel_bound


# =========================================================================================================== tables
def _rotvec(rng, F, scale):
    v = rng.standard_normal((F, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (scale * rng.random((F, 1)))


def _var(rng, dim, F):
    if dim == 2:
        return rng.uniform(-5.0, 5.0, (F, 2))
    if dim == 3:
        return np.concatenate([rng.uniform(-5.0, 5.0, (F, 2)), rng.uniform(-np.pi, np.pi, (F, 1))], axis=1)
    return np.concatenate([rng.uniform(-5.0, 5.0, (F, 3)), _rotvec(rng, F, 2.5)], axis=1)


def geometry_table(family, F=129, seed=0):
    """F generic pairs: translations within +-5, headings over the circle, rotation vectors up to 2.5 rad (relative rotations then stay
    clear of pi by more than 0.1: the table's worst case is 2 x 2.5 about opposite axes = 5 rad = 2 pi - 1.28, angle 1.28)"""
    rng = np.random.default_rng(20260 + seed + sum(map(ord, family)))
    _, _, da, db, _ = FAMILIES[family]
    A, B = _var(rng, da, F), _var(rng, db, F)
    if da == 6:   # keep every relative rotation at least 0.2 rad from pi: halve the second rotation of a row that comes closer
        ang = np.linalg.norm(_np_so3_log(np.swapaxes(_np_so3_exp(A[:, 3:]), -1, -2) @ _np_so3_exp(B[:, 3:])), axis=1)
        B[ang > np.pi - 0.2, 3:] *= 0.5
    return A, B


def blocks(X, C, N):
    """C * N rows of coordinates -> SoA blocks (C, dim, N): row c * N + i is particle i of block c"""
    X = np.asarray(X, dtype=np.float64)
    return np.ascontiguousarray(X.reshape(C, N, X.shape[1]).transpose(0, 2, 1))


def rows_of(blk):
    """SoA blocks (C, dim, N) -> C * N rows"""
    blk = np.asarray(blk)
    return np.ascontiguousarray(blk.transpose(0, 2, 1).reshape(-1, blk.shape[1]))


def pose2_edge_table():
    """Pose2Pose2 pairs at the heading edges: differences of +-pi, +-(pi - 1e-12), headings 3 pi and -7.5"""
    rows = []
    for thp, thq in ((0.0, np.pi), (0.0, -np.pi), (0.3, 0.3 + np.pi - 1e-12), (0.3, 0.3 - np.pi + 1e-12), (3.0 * np.pi, 0.1), (-7.5, 2.0),
                     (3.0 * np.pi, -7.5), (1.0, 1.0), (np.pi, -np.pi)):
        rows.append(([1.0, -2.0, thp], [3.5, 0.25, thq]))
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def landmark_edge_table():
    """(pose, landmark) pairs with the landmark 1e-6 .. 1e6 away, in several directions"""
    A, B = [], []
    for k, dist in enumerate((1e-6, 1e-3, 1.0, 1e3, 1e6)):
        for beta in (0.1, 2.0, -3.0):
            pose = [0.5, -0.25, 0.7 * (k - 2)]
            A.append(pose); B.append([pose[0] + dist * np.cos(beta), pose[1] + dist * np.sin(beta)])
    return np.array(A), np.array(B)


def pose3_edge_table():
    """Pose3 pairs whose relative rotation is 0, 1e-9, 1 and pi - 1e-3 about generic and coordinate axes (q = p o (t, Exp(angle axis))),
    and rotation vectors beyond the principal range on the inputs (|w| up to 3 pi)"""
    rng = np.random.default_rng(77)
    A, B = [], []
    axes = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])] + [v / np.linalg.norm(v) for v in rng.standard_normal((3, 3))]
    for ang in (0.0, 1e-9, 1.0, np.pi - 1e-3):
        for ax in axes:
            wp = _rotvec(rng, 1, 2.0)[0]
            Rq = _np_so3_exp(wp) @ _np_so3_exp(ang * ax)
            A.append(np.concatenate([rng.uniform(-3, 3, 3), wp])); B.append(np.concatenate([rng.uniform(-3, 3, 3), _np_so3_log(Rq)]))
    for scale in (1.5 * np.pi, 2.5 * np.pi, 3.0 * np.pi):
        for ax in axes[3:]:
            A.append(np.concatenate([rng.uniform(-3, 3, 3), scale * ax])); B.append(np.concatenate([rng.uniform(-3, 3, 3), 0.4 * axes[4] + 0.1 * ax]))
    return np.array(A), np.array(B)


def near_pi_rows(A, B):
    """rows of a Pose3 table whose relative rotation is within 0.01 of pi"""
    ang = np.linalg.norm(_np_so3_log(np.swapaxes(_np_so3_exp(A[:, 3:]), -1, -2) @ _np_so3_exp(B[:, 3:])), axis=1)
    return np.nonzero(ang > np.pi - 0.01)[0]


# =========================================================================================================== the reference's line, restated
def np_mmd_pose2(a, b, bw=0.001):
    """the biased V-statistic of rome_mmd on two (3, N) Pose2 coordinate sets (include/rome_mi355.h), in NumPy"""
    def S(x, y):
        d = x[:, :, None] - y[:, None, :]
        d[2] = np.arctan2(np.sin(d[2]), np.cos(d[2]))
        return np.exp(-bw * (d * d).sum(0)).sum()
    na, nb = a.shape[1], b.shape[1]
    return S(a, a) / na ** 2 - 2.0 * S(a, b) / (na * nb) + S(b, b) / nb ** 2
