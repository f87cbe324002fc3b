"""References for the partial rotation factor Pose3Pose3Rotation (RoME src/factors/PartialPose3.jl:204-227).  Nothing here comes from the
kernel.

Three sides:
  * mp_residual / mp_root -- mpmath at 50 digits, from rotation matrices: r = z - Log(R_p^T R_q) with lin_ref's _so3_exp / _so3_log (the
                             logarithm through atan2, accurate at every angle below pi); the root R_F Exp(+-z) as the matrix product, then
                             the logarithm, rounded once.
  * np_residual / np_root -- float64 NumPy restatement of both (lin_ref's _np_so3_exp / _np_so3_log: Manifolds' exp / log forms).
  * rot_row / rot_conv    -- the convolution loop (measurement, nullhypo draw, cycles x {entropy, solve}, status, nullhypo spread) built
                             from the oracle's primitives the way partial3_ref.xyy_row is; Nelder-Mead through ro.nelder_mead on a cost made
                             of ro.so3_exp / ro.so3_log.

Rules (include/rome_mi355.h):
  residual r = z - Log(R_p^T R_q), Log the principal rotation vector; translations do not enter.
  root     dir 0: R_q = R_p Exp(z); dir 1: R_p = R_q Exp(-z); the target's translation passes through; the stored coordinates are the
           principal rotation vector.  For |z| >= pi the functor has no zero and every status output says 1.
  entropy  additive on coordinates 3, 4, 5 from the d = 6 uniforms; the spread over all six coordinates.

Tolerances (class Table, the rule of lin_ref.Reference): per table, the deviation of the float64 restatement from mp, per row, relative
to max(1, largest |reference entry| of the row); the kernel's bound is 8x that figure with a floor of 64 ulp.
"""
import functools
import math

import mpmath as mpm
import numpy as np

from lin_ref import (_so3_exp, _so3_log, _mm, _mt, _np_so3_exp, _np_so3_log, pose3_compose, row_scale, AXES, POSE_NORMS, DPS, EPS)

CLOSED_FORM, NEWTON, NELDER_MEAD, GAUSS_NEWTON = 0, 1, 2, 3
ROT_PARTIAL = (3, 4, 5)                      # 0-based coordinates of partial = (4, 5, 6)
RESIDUAL_ANGLES = {"phi_tiny": (0.0, 1e-12, 1e-6), "phi_mid": (0.1, 1.0, 3.0), "near_pi_1e-3": (math.pi - 1e-3,)}


# =========================================================================================================== mpmath side
def _mpv(v):
    return [mpm.mpf(float(x)) for x in v]


def _frame_mp(pose):
    """rotation of a pose given as coordinates (6; Exp of the rotation vector) or as a native point (12; the column-major entries taken
    exactly) -> 3x3 list of mpf"""
    pose = np.asarray(pose, dtype=np.float64)
    if pose.size == 6:
        return _so3_exp(_mpv(pose[3:]))
    return [[mpm.mpf(float(pose[3 + i + 3 * j])) for j in range(3)] for i in range(3)]


def mp_residual(z, p, q):
    """rows: z (n, 3), p / q (n, 6) or (n, 12) -> (n, 3) float64, each entry rounded once"""
    z, p, q = np.atleast_2d(z), np.atleast_2d(p), np.atleast_2d(q)
    out = np.empty((len(z), 3))
    with mpm.workdps(DPS):
        for i in range(len(z)):
            w = _so3_log(_mm(_mt(_frame_mp(p[i])), _frame_mp(q[i])))
            out[i] = [float(a - b) for a, b in zip(_mpv(z[i]), w)]
    return out


def mp_root(dirs, z, fixed):
    """rows: dirs (n,), z (n, 3), fixed (n, 6) coordinates -> (n, 3): the principal rotation vector of R_F Exp(z) (dir 0) / R_F Exp(-z) (dir 1)"""
    z, fixed = np.atleast_2d(z), np.atleast_2d(fixed)
    dirs = np.broadcast_to(np.asarray(dirs), (len(z),))
    out = np.empty((len(z), 3))
    with mpm.workdps(DPS):
        for i in range(len(z)):
            s = -1 if dirs[i] else 1
            out[i] = [float(v) for v in _so3_log(_mm(_frame_mp(fixed[i]), _so3_exp([s * v for v in _mpv(z[i])])))]
    return out


# =========================================================================================================== float64 NumPy restatement
def _frame_np(pose):
    pose = np.asarray(pose, dtype=np.float64)
    if pose.shape[-1] == 6:
        return _np_so3_exp(pose[..., 3:])
    return np.swapaxes(pose[..., 3:].reshape(pose.shape[:-1] + (3, 3)), -1, -2)      # column-major entries


def np_residual(z, p, q):
    z, p, q = np.atleast_2d(np.asarray(z, dtype=np.float64)), np.atleast_2d(p), np.atleast_2d(q)
    with np.errstate(all="ignore"):
        return z - _np_so3_log(np.swapaxes(_frame_np(p), -1, -2) @ _frame_np(q))


def np_root(dirs, z, fixed):
    z = np.asarray(z, dtype=np.float64)
    sg = np.where(np.asarray(dirs) != 0, -1.0, 1.0)
    sg = sg[..., None] if np.ndim(sg) else sg
    with np.errstate(all="ignore"):
        return _np_so3_log(_frame_np(fixed) @ _np_so3_exp(sg * z))


def points(coords):
    """native points [t(3), R column-major(9)] of pose coordinates (n, 6), in float64 (the restatement's Exp)"""
    coords = np.asarray(coords, dtype=np.float64)
    R = _np_so3_exp(coords[..., 3:])
    return np.concatenate([coords[..., :3], np.swapaxes(R, -1, -2).reshape(coords.shape[:-1] + (9,))], axis=-1)


# =========================================================================================================== tables and bounds
class Table:
    """One table of rows with its mp reference, the restatement, the reference-side error figure and the kernel's bound."""

    def __init__(self, ref, np_side):
        self.ref = np.asarray(ref)
        self.np = np.asarray(np_side)
        self.scale = row_scale(self.ref)
        self.figure = float((np.abs(self.np - self.ref).reshape(len(self.ref), -1).max(axis=1) / self.scale).max())
        self.rel_bound = max(8.0 * self.figure, 64.0 * EPS)

    def check(self, got, rows=None):
        """kernel output against mp -> (largest deviation / row scale, the bound it must not exceed)"""
        ref, scale = (self.ref, self.scale) if rows is None else (self.ref[rows], self.scale[rows])
        d = np.abs(np.asarray(got) - ref).reshape(len(ref), -1).max(axis=1)
        return float((d / scale).max()), self.rel_bound


def _stack(rows):
    z, p, q = (np.array([r[k] for r in rows], dtype=np.float64) for k in range(3))
    return dict(z=z, p=p, q=q, p_pt=points(p), q_pt=points(q))


def residual_tables():
    """group name -> dict(z, p, q, p_pt, q_pt).  Residual rotations of 0, 1e-12, 1e-6, 0.1, 1, 3 and pi - 1e-3 about generic and coordinate
    axes (one group per error regime of the shared log formula, as lin_ref.PHI_GROUPS), pose rotation vectors of norm 0, 1e-9, pi - 1e-6,
    4 and 7 on either pose, and 40 seeded generic rows."""
    rng = np.random.default_rng(9100)
    g = {}
    for name, angles in RESIDUAL_ANGLES.items():
        rows = []
        for ax in AXES:
            p = np.concatenate([rng.standard_normal(3) * 4, rng.standard_normal(3) * 0.6])
            z = rng.standard_normal(3)
            dt = rng.standard_normal(3)
            for a in angles:
                rows.append((z, p, pose3_compose(p, np.concatenate([dt, a * ax]))))         # Log(R_p^T R_q) = a * ax
        g[name] = _stack(rows)
    rows = []
    for nrm in POSE_NORMS:
        far = np.concatenate([rng.standard_normal(3) * 4, nrm * AXES[0]])
        d = np.concatenate([rng.standard_normal(3), 0.4 * np.array([0.6, 0.0, -0.8])])
        z = rng.standard_normal(3)
        rows.append((z, far, pose3_compose(far, d)))                                        # the extreme vector as p ...
        rows.append((z, pose3_compose(far, d), far))                                        # ... and as q
    g["pose_coords"] = _stack(rows)
    rows = []
    for _ in range(40):
        p = np.concatenate([rng.standard_normal(3) * 10, rng.standard_normal(3) * 0.8])
        q = pose3_compose(p, np.concatenate([rng.standard_normal(3), rng.standard_normal(3) * 0.7]))
        rows.append((rng.standard_normal(3) * 0.7, p, q))
    g["generic"] = _stack(rows)
    return g


@functools.lru_cache(maxsize=None)
def residual_references():
    """group name -> (table, Table of the coordinate layout, Table of the point layout)"""
    out = {}
    for name, t in residual_tables().items():
        out[name] = (t, Table(mp_residual(t["z"], t["p"], t["q"]), np_residual(t["z"], t["p"], t["q"])),
                     Table(mp_residual(t["z"], t["p_pt"], t["q_pt"]), np_residual(t["z"], t["p_pt"], t["q_pt"])))
    return out


def root_table(n=48, seed=9200):
    """seeded root rows: dirs, z with |z| <= 3, fixed poses; rows whose root rotation lies within 0.05 of pi are redrawn (the principal
    vector flips sign there)"""
    rng = np.random.default_rng(seed)
    dirs, zs, fx = [], [], []
    while len(zs) < n:
        z = rng.standard_normal(3)
        z *= rng.uniform(0.0, 3.0) / np.linalg.norm(z)
        f = np.concatenate([rng.standard_normal(3) * 10, rng.standard_normal(3) * 0.8])
        d = int(rng.integers(0, 2))
        if abs(np.linalg.norm(np_root(d, z, f)) - math.pi) < 0.05:
            continue
        dirs.append(d); zs.append(z); fx.append(f)
    return dict(dirs=np.array(dirs, dtype=np.int32), z=np.array(zs), fixed=np.array(fx))


@functools.lru_cache(maxsize=None)
def root_reference():
    t = root_table()
    return t, Table(mp_root(t["dirs"], t["z"], t["fixed"]), np_root(t["dirs"], t["z"], t["fixed"]))


def subset(N, seed=0):
    """the particles of a block of N that the mp reference serves: the lane-block edges plus 8 seeded ones"""
    fixed = [0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 511, 512, N - 2, N - 1]
    rnd = np.random.default_rng(2000 + seed).integers(0, N, 8).tolist()
    return sorted({i for i in fixed + rnd if 0 <= i < N})


# =========================================================================================================== the convolution loop
def measurement(mu, L, xi):
    """z = mu + L xi, L the packed lower Cholesky factor [6] (the d = 3 normal rule of Pose3Pose3XYYaw)"""
    return np.array([mu[0] + L[0] * xi[0], mu[1] + L[1] * xi[0] + L[2] * xi[1], mu[2] + L[3] * xi[0] + L[4] * xi[1] + L[5] * xi[2]])


class _Cost:
    """sum r^2 of one particle over the target's rotation vector, through the oracle's ro.so3_exp / ro.so3_log on preallocated buffers"""

    def __init__(self):
        import oracle as ro
        self.w, self.T, self.U, self.l = np.zeros(3), np.zeros(9), np.zeros(9), np.zeros(3)
        P = ro.C.POINTER(ro.C.c_double)
        self.pw, self.pT, self.pU, self.pl = (a.ctypes.data_as(P) for a in (self.w, self.T, self.U, self.l))
        self.exp, self.log = ro.lib().ro_so3_exp, ro.lib().ro_so3_log

    def frame(self, w):
        self.w[:] = w
        self.exp(self.pw, self.pT)
        return self.T.reshape(3, 3).T.copy()

    def __call__(self, dirn, z, F, x):
        T = self.frame(x)
        U = F.T @ T if dirn == 0 else T.T @ F
        self.U[:] = U.T.ravel()
        self.log(self.pU, self.pl)
        r = z - self.l
        return float(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])


_cost = None


def rot_row(opts, dirn, mu, cov, fixed, target, stream, solver, noise=None, noise_is_meas=False, nullhypo=0.0, spread_nh=3.0,
            tol=None, max_iters=None):
    """One Pose3Pose3Rotation row.  fixed / target [6][N] -> (out [6][N], status [N], z [N][3]).  CLOSED_FORM / NEWTON / GAUSS_NEWTON return
    the float64 restatement of the root (np_root); status is the functor's (np_residual) at the returned point."""
    import oracle as ro
    import partial3_ref as p3
    global _cost
    if _cost is None:
        _cost = _Cost()
    N, seed = opts.n_particles, opts.seed
    cycles = max(1, opts.inflate_cycles) if solver == NELDER_MEAD else 1
    tol = (1e-8 if solver == NELDER_MEAD else 1e-12) if tol is None else tol
    max_iters = (1000 if solver == NELDER_MEAD else 20) if max_iters is None else max_iters
    L = ro.cholesky_lower(np.asarray(cov, dtype=np.float64))
    out = np.array(target, dtype=np.float64, copy=True)
    status = np.zeros(N, dtype=np.int32)
    z = np.empty((N, 3))
    for i in range(N):
        xi = np.asarray(noise[:, i], dtype=np.float64) if noise is not None else ro.rng_normals(seed, stream, i, 3)
        z[i] = xi if noise_is_meas else measurement(mu, L, xi)
    nullh, nh_u, nh_spread = np.zeros(N, dtype=bool), None, 0.0
    if nullhypo > 0.0:
        nh_spread = spread_nh * p3.frechet_std(out) if N > 1 else 0.0
        nullh, nh_u = p3._nullhypo_draws(seed, stream, N, nullhypo)
    live = ~nullh
    if solver != NELDER_MEAD:
        root = np_root(dirn, z, fixed.T)
        out[3:6, live] = root.T[:, live]
    else:
        F = [_cost.frame(fixed[3:6, i]) for i in range(N)]
        for cyc in range(cycles):
            spread = opts.inflation * p3.frechet_std(out) if (opts.inflation > 0.0 and N > 1) else 0.0
            for i in range(N):
                if nullh[i]:
                    continue
                t = out[:, i].copy()
                if spread > 0.0:
                    p3._add_entropy(t, spread, ro.rng_entropy(seed, stream, i, cyc, 6), ROT_PARTIAL)
                x, rc, _ = ro.nelder_mead(lambda x, zz=z[i], f=F[i]: _cost(dirn, zz, f, x), t[3:6], max_iters, tol)
                t[3:6] = x
                out[:, i] = t
                status[i] = 1 if rc else 0
    if solver != NELDER_MEAD:
        r = np_residual(z, fixed.T, out.T) if dirn == 0 else np_residual(z, out.T, fixed.T)
        status[live] = (np.abs(r).max(axis=1) > tol)[live]
    if nh_spread > 0.0:
        for i in range(N):
            if nullh[i]:
                t = out[:, i].copy()
                p3._add_entropy(t, nh_spread, nh_u[i], ROT_PARTIAL)
                out[:, i] = t
    return out, status, z


def rot_conv(opts, dirs, mu, cov, fixed, target, solver, noise=None, **kw):
    """C rows: dirs [C], mu [C][3], cov [C][3][3], fixed / target [C][6][N], noise [C][3][N] or None -> (out, status, z [C][N][3])"""
    res = [rot_row(opts, int(dirs[c]), mu[c], cov[c], np.asarray(fixed[c]), np.asarray(target[c]), opts.stream_offset + c, solver,
                   None if noise is None else np.asarray(noise[c]), **kw) for c in range(len(mu))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


# =========================================================================================================== the fixture
def make_fixture():
    """the data of tests/golden/rotation3_kats.json (python tests/rotation3_ref.py writes it)"""
    phi = 0.1
    rpys = [[0, 0, 0], [phi, 0, 0], [0, phi, 0], [0, 0, phi], [-phi, 0, 0], [0, -phi, 0], [0, 0, -phi]]
    kats = []
    for rpy in rpys:                    # RotXYZ(r, p, y) = Rx(r) Ry(p) Rz(y): with one angle non-zero it is the rotation by it about that axis
        w = np.array(rpy, dtype=np.float64)
        q = points(np.concatenate([np.zeros(3), w])[None])[0]
        kats.append(dict(rpy=[float(v) for v in rpy], z=[float(v) for v in rpy], p=points(np.zeros((1, 6)))[0].tolist(), q=q.tolist()))
    rt, rref = root_reference()
    g = residual_references()["generic"]
    return {
        "provenance": "data only.  kats and packing: the cases of the reference's tests, transcribed (file:line in `source`).  residual_rows "
                      "and root_rows: seeded rows (residual_tables()['generic'], root_table()) with their mpmath answers at 50 digits, each "
                      "rounded once.  Written by `python tests/rotation3_ref.py`; tests/test_rotation3_host.py regenerates and compares it.",
        "kats": {"source": "test/testPartialPose3.jl:520-547", "norm_below": 1e-10, "cases": kats},
        "packing": {"source": "test/testpackingconverters.jl:256-264", "mu": [0.1, 0.2, 0.3], "cov": (0.1 * np.eye(3)).tolist()},
        "residual_rows": {"z": g[0]["z"].tolist(), "p": g[0]["p"].tolist(), "q": g[0]["q"].tolist(), "mp": g[1].ref.tolist()},
        "root_rows": {"dirs": rt["dirs"].tolist(), "z": rt["z"].tolist(), "fixed": rt["fixed"].tolist(), "mp": rref.ref.tolist()},
    }


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotation3_kats.json")
    with open(path, "w") as f:
        json.dump(make_fixture(), f, indent=1)
        f.write("\n")
    print("wrote", path)
