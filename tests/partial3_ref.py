"""Per-row restatement of the partial Pose3 factor convolutions (Pose3Pose3XYYaw, PriorPose3ZRP; RoME src/factors/PartialPose3.jl), built
from the oracle's exported primitives -- ro.rng_normals(..., 3), ro.rng_entropy(..., 6), ro.belief_spread, ro.nelder_mead, ro.philox,
ro.so3_exp / ro.so3_log, ro.residual_pose2pose2 -- with the scalar yaw root evaluated in mpmath at 50 digits and rounded once.
The loop is shaped after tests/range_ref.py / bearing_ref.py: measurement, start copy, nullhypo draw, cycles x {entropy, solve}, status,
nullhypo spread.

Rules (include/rome_mi355.h):
  yaw of a Pose3: psi(R) = atan2(R21, R11), R11 = R21 = 0 -> 0.
  Pose3Pose3XYYaw: r = the Pose2Pose2 residual of (z, p2, q2), p2 = (p.t_xy, psi(R_p)).  Unknowns (x, y, w_z) of the target, its
    z, w_x, w_y pass through.  psi*, t*: dir 0 psi* = psi_p + z_th, t* = p.t_xy + R2(psi_p) z_xy; dir 1 psi* = psi_q - z_th,
    t* = q.t_xy - R2(psi_p) z_xy with psi_p the yaw of the returned p.  w_z = s solves g(s) = wrap(psi(Exp(w_x, w_y, s)) - psi*) = 0 by Newton
    (dpsi/ds from dR = hat(J_l e3) R = R hat(J_r e3)): CLOSED_FORM / NEWTON from wrap(psi*); GAUSS_NEWTON from the start particle's w_z with
    the functor at every iterate; NELDER_MEAD on sum r^2 over (x, y, w_z), the only solver that runs the inflation cycles.
  entropy: ADDITIVE on the partial coordinates, from the d = 6 uniforms (three of them used); spread over all six coordinates.
  PriorPose3ZRP: z_s = mu_z + sigma_z xi0, (r, p) = mu_rp + L_rp (xi1, xi2), R = R_y(p) R_x(r), w = Log R; coordinates 3, 4, 5 of the
    target's own particle <- (z_s, w_x, w_y)."""
import math

import mpmath as mp
import numpy as np

import oracle as ro

mp.mp.dps = 50
CLOSED_FORM, NEWTON, NELDER_MEAD, GAUSS_NEWTON = 0, 1, 2, 3
XYY_PARTIAL, ZRP_PARTIAL = (0, 1, 5), (2, 3, 4)     # 0-based coordinates of partial = (1, 2, 6) and (3, 4, 5)


def wrap(a):
    return math.remainder(a, 2.0 * math.pi)


def _wrap_mp(a):
    return a - 2 * mp.pi * mp.nint(a / (2 * mp.pi))


def _col1_mp(w):
    """first column (R11, R21, R31) of Exp(w) and u = J_l(w) e3, in mpmath"""
    x, y, z = (mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in w)
    th2 = x * x + y * y + z * z
    if th2 == 0:
        a, b, k = mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
    else:
        th = mp.sqrt(th2)
        a, b, k = mp.sin(th) / th, (1 - mp.cos(th)) / th2, (th - mp.sin(th)) / (th2 * th)
    c = (1 + b * (x * x - th2), a * z + b * x * y, -a * y + b * x * z)
    u = (b * y + k * x * z, -b * x + k * y * z, 1 - k * (x * x + y * y))
    return c, u


def _yaw_mp(c):
    return mp.atan2(c[1], c[0]) if (c[0] != 0 or c[1] != 0) else mp.mpf(0)


def _rate_mp(c, u):
    n2 = c[0] * c[0] + c[1] * c[1]
    return u[2] - c[2] * (u[0] * c[0] + u[1] * c[1]) / n2 if n2 > 0 else mp.mpf(1)


def yaw(w):
    """psi of the rotation vector w, rounded once"""
    return float(_yaw_mp(_col1_mp(w)[0]))


def yaw_of_point(pt):
    """psi of a native point [t(3), R column-major(9)]"""
    r11, r21 = float(pt[3]), float(pt[4])
    return math.atan2(r21, r11) if (r11 != 0.0 or r21 != 0.0) else 0.0


def project(pose):
    """Pose3 coordinates (6) or native point (12) -> its SE(2) projection (x, y, psi)"""
    pose = np.asarray(pose, dtype=np.float64)
    return np.array([pose[0], pose[1], yaw(pose[3:6]) if pose.size == 6 else yaw_of_point(pose)])


def residual(z, p, q):
    """rows: z (n, 3), p / q (n, 6) coordinates or (n, 12) native points -> (n, 3): the oracle's Pose2Pose2 residual of the projections"""
    z, p, q = np.atleast_2d(z), np.atleast_2d(p), np.atleast_2d(q)
    return ro.residual_pose2pose2(z, np.array([project(r) for r in p]), np.array([project(r) for r in q]))


def _col1_d(x, y, z):
    """first column of Exp(w) and u = J_l(w) e3 in double precision (series below |w|^2 = 1e-2)"""
    th2 = x * x + y * y + z * z
    if th2 < 1e-2:
        a = 1.0 - th2 / 6.0 + th2 * th2 / 120.0 - th2 ** 3 / 5040.0 + th2 ** 4 / 362880.0
        b = 0.5 - th2 / 24.0 + th2 * th2 / 720.0 - th2 ** 3 / 40320.0
        k = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0 - th2 ** 3 / 362880.0
    else:
        th = math.sqrt(th2)
        a, b, k = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    return ((1.0 + b * (x * x - th2), a * z + b * x * y, -a * y + b * x * z),
            (b * y + k * x * z, -b * x + k * y * z, 1.0 - k * (x * x + y * y)))


def _newton(dirn, z, F2, t, s0, max_iters, tol, functor):
    """Newton on s from s0 -> (x, y, s, status).  F2: the fixed pose's projection.  The iteration itself runs in double precision (it only
    selects the branch and decides the status); a converged particle is then polished to the exact root of that branch in mpmath and
    rounded once.  A particle at the cap returns its last iterate."""
    back = dirn != 0
    psi_star = F2[2] - z[2] if back else F2[2] + z[2]
    wx, wy = float(t[3]), float(t[4])

    def xy(psi, M=math):
        cF, sF = M.cos(F2[2]), M.sin(F2[2])
        if back:
            return F2[0] - (M.cos(psi) * z[0] - M.sin(psi) * z[1]), F2[1] - (M.sin(psi) * z[0] + M.cos(psi) * z[1])
        return F2[0] + (cF * z[0] - sF * z[1]), F2[1] + (sF * z[0] + cF * z[1])

    def ev(s):
        c, u = _col1_d(wx, wy, s)
        n2 = c[0] * c[0] + c[1] * c[1]
        psi = math.atan2(c[1], c[0]) if n2 > 0.0 else 0.0
        rate = u[2] - c[2] * (u[0] * c[0] + u[1] * c[1]) / n2 if n2 > 0.0 else 1.0
        return wrap(psi - psi_star), rate, psi

    s = wrap(psi_star) if s0 is None else float(s0)
    done = False
    for _ in range(max_iters):
        g, rate, psi = ev(s)
        if functor:
            T2 = [*xy(psi), psi]
            r = ro.residual_pose2pose2([z], [F2], [T2])[0] if not back else ro.residual_pose2pose2([z], [T2], [F2])[0]
            done = np.abs(r).max() <= tol
        else:
            done = abs(g) <= tol
        if done:
            break
        s -= g / (rate if abs(rate) > 1e-6 else 1.0)
    if not done:
        x, y = xy(ev(s)[2])
        return x, y, s, 1
    F2 = [mp.mpf(float(v)) for v in F2]
    z = [mp.mpf(float(v)) for v in z]
    psi_star = F2[2] - z[2] if back else F2[2] + z[2]
    s = mp.mpf(s)
    for _ in range(6):     # the exact root of this branch
        c, u = _col1_mp((mp.mpf(wx), mp.mpf(wy), s))
        psi = _yaw_mp(c)
        g = _wrap_mp(psi - psi_star)
        if abs(g) < mp.mpf("1e-40"):
            break
        s -= g / _rate_mp(c, u)
    x, y = xy(psi, mp)
    return float(x), float(y), float(s), 0


class _P2P2:
    """ro.residual_pose2pose2 of ONE row through preallocated buffers (the Nelder-Mead cost calls it thousands of times per row)"""

    def __init__(self):
        self.buf = np.zeros((4, 3))
        self.ptr = [self.buf[k].ctypes.data_as(ro.C.POINTER(ro.C.c_double)) for k in range(4)]
        self.fn = ro.lib().ro_residual_pose2pose2

    def __call__(self, z, p2, q2):
        self.buf[0], self.buf[1], self.buf[2] = z, p2, q2
        self.fn(1, self.ptr[0], self.ptr[1], self.ptr[2], self.ptr[3])
        return self.buf[3]


_p2p2 = None


def _cost(dirn, z, F2, wx, wy, x):
    global _p2p2
    if _p2p2 is None:
        _p2p2 = _P2P2()
    T2 = (x[0], x[1], _yaw_fast(wx, wy, x[2]))
    r = _p2p2(z, F2, T2) if dirn == 0 else _p2p2(z, T2, F2)
    return float(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])


def _yaw_fast(x, y, z):
    """psi in double precision (the Nelder-Mead cost: thousands of evaluations per row)"""
    c, _ = _col1_d(x, y, z)
    return math.atan2(c[1], c[0]) if (c[0] != 0.0 or c[1] != 0.0) else 0.0


def frechet_std(blk):
    """IIF calcStdBasicSpread over all six coordinates: root of the summed coordinate variances, "no std yet -> 1" """
    _, sd = ro.belief_spread(blk)
    v = math.sqrt(float(np.sum(sd * sd)))
    return v if v > 1e-10 else 1.0


def _uniforms(words):
    return [((w + 0.5) / 4294967296.0) for w in words]


def _nullhypo_draws(seed, stream, N, nullhypo):
    key = [seed & 0xFFFFFFFF, seed >> 32]
    nullh = np.zeros(N, dtype=bool)
    u = np.zeros((N, 6))
    for i in range(N):
        w0 = ro.philox([i, stream & 0xFFFFFFFF, stream >> 32, 5 << 16], key)
        w1 = ro.philox([i, stream & 0xFFFFFFFF, stream >> 32, (5 << 16) | 1], key)
        nullh[i] = _uniforms([w0[0]])[0] < nullhypo
        u[i] = _uniforms(w0[1:4]) + _uniforms(w1[0:3])
    return nullh, u


def _add_entropy(t, spread, u, partial):
    for k in partial:
        t[k] += spread * (u[k] - 0.5)


def xyy_measurement(mu, L, xi):
    """z = mu + L xi, L the packed lower Cholesky factor [6]"""
    return np.array([mu[0] + L[0] * xi[0], mu[1] + L[1] * xi[0] + L[2] * xi[1], mu[2] + L[3] * xi[0] + L[4] * xi[1] + L[5] * xi[2]])


def xyy_row(opts, dirn, mu, cov, fixed, target, stream, solver, noise=None, noise_is_meas=False, nullhypo=0.0, spread_nh=3.0,
            tol=None, max_iters=None):
    """One Pose3Pose3XYYaw row.  fixed / target [6][N] -> (out [6][N], status [N]); noise [3][N] or None."""
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
        z[i] = xi if noise_is_meas else xyy_measurement(mu, L, xi)
    F2 = [project(fixed[:, i]) for i in range(N)]
    nullh, nh_u, nh_spread = np.zeros(N, dtype=bool), None, 0.0
    if nullhypo > 0.0:
        nh_spread = spread_nh * frechet_std(out) if N > 1 else 0.0
        nullh, nh_u = _nullhypo_draws(seed, stream, N, nullhypo)
    for cyc in range(cycles):
        spread = opts.inflation * frechet_std(out) if (solver == NELDER_MEAD and opts.inflation > 0.0 and N > 1) else 0.0
        for i in range(N):
            if nullh[i]:
                continue
            t = out[:, i].copy()
            if spread > 0.0:
                _add_entropy(t, spread, ro.rng_entropy(seed, stream, i, cyc, 6), XYY_PARTIAL)
            if solver == NELDER_MEAD:
                x, rc, _ = ro.nelder_mead(lambda x, zz=z[i], f=F2[i], wx=t[3], wy=t[4]: _cost(dirn, zz, f, wx, wy, x), [t[0], t[1], t[5]],
                                          max_iters, tol)
                t[0], t[1], t[5] = x
                st = 1 if rc else 0
            else:
                s0 = t[5] if solver == GAUSS_NEWTON else None
                t[0], t[1], t[5], st = _newton(dirn, z[i], F2[i], t, s0, max_iters, tol, functor=solver == GAUSS_NEWTON)
            out[:, i] = t
            status[i] = st
    if solver == NEWTON:
        for i in range(N):
            if not nullh[i]:
                r = residual([z[i]], [fixed[:, i]], [out[:, i]]) if dirn == 0 else residual([z[i]], [out[:, i]], [fixed[:, i]])
                status[i] = 0 if np.abs(r).max() <= tol else 1
    if nh_spread > 0.0:
        for i in range(N):
            if nullh[i]:
                t = out[:, i].copy()
                _add_entropy(t, nh_spread, nh_u[i], XYY_PARTIAL)
                out[:, i] = t
    return out, status, z


def xyy_conv(opts, dirs, mu, cov, fixed, target, solver, noise=None, **kw):
    """C rows: dirs [C], mu [C][3], cov [C][3][3], fixed / target [C][6][N], noise [C][3][N] or None -> (out, status, z [C][N][3])"""
    res = [xyy_row(opts, int(dirs[c]), mu[c], cov[c], np.asarray(fixed[c]), np.asarray(target[c]), opts.stream_offset + c, solver,
                   None if noise is None else np.asarray(noise[c]), **kw) for c in range(len(mu))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


def zrp_sample(mu, sigma_z, L_rp, xi):
    """(z_s, w_x, w_y) of one particle: R = R_y(p) R_x(r) as a unit quaternion on half angles, w = Log R (mpmath, rounded once)"""
    r = mp.mpf(float(mu[1] + L_rp[0] * xi[1]))
    p = mp.mpf(float(mu[2] + L_rp[1] * xi[1] + L_rp[2] * xi[2]))
    cr, sr, cp, sp = mp.cos(r / 2), mp.sin(r / 2), mp.cos(p / 2), mp.sin(p / 2)
    w, x, y, z = cp * cr, cp * sr, sp * cr, -sp * sr
    n = mp.sqrt(x * x + y * y + z * z)
    k = 2 * mp.atan2(n, w) / n if n > 0 else mp.mpf(2)
    return np.array([mu[0] + sigma_z * xi[0], float(k * x), float(k * y)])


def zrp_row(opts, mu, sigma_z, cov_rp, target, stream, noise=None, noise_is_meas=False, nullhypo=0.0, spread_nh=3.0):
    """One PriorPose3ZRP row: target [6][N] -> out [6][N] (coordinates 2, 3, 4 replaced)"""
    N, seed = opts.n_particles, opts.seed
    L = ro.cholesky_lower(np.asarray(cov_rp, dtype=np.float64))
    out = np.array(target, dtype=np.float64, copy=True)
    nullh, nh_u, nh_spread = np.zeros(N, dtype=bool), None, 0.0
    if nullhypo > 0.0:
        nh_spread = spread_nh * frechet_std(out) if N > 1 else 0.0
        nullh, nh_u = _nullhypo_draws(seed, stream, N, nullhypo)
    for i in range(N):
        xi = np.asarray(noise[:, i], dtype=np.float64) if noise is not None else ro.rng_normals(seed, stream, i, 3)
        s = xi if noise_is_meas else zrp_sample(mu, sigma_z, L, xi)
        if nullh[i]:
            if nh_spread > 0.0:
                t = out[:, i].copy()
                _add_entropy(t, nh_spread, nh_u[i], ZRP_PARTIAL)
                out[:, i] = t
        else:
            out[2:5, i] = s
    return out


def zrp_conv(opts, mu, sigma_z, cov_rp, target, noise=None, **kw):
    return np.stack([zrp_row(opts, mu[c], float(sigma_z[c]), cov_rp[c], np.asarray(target[c]), opts.stream_offset + c,
                             None if noise is None else np.asarray(noise[c]), **kw) for c in range(len(mu))])
