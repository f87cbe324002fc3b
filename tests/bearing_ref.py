"""Per-row restatement of the bearing-only factor convolution (Pose2Point2Bearing; RoME src/factors/Bearing2D.jl), built only from the
oracle's exported primitives: ro.rng_normals(..., 1), ro.rng_entropy, ro.belief_spread, ro.nelder_mead, ro.philox, and
ro.residual_pose2point2br for the residual (its component 0 IS the bearing-only residual, BearingRange2D.jl:57-60).
The loop is shaped after tests/range_ref.py: measurement, start copy, nullhypo draw, cycles x {entropy, solve}, status, nullhypo spread.

Rules (include/rome_mi355.h): r = sym_rem(b − atan2(pl)), pl = R(θp)ᵀ (l − p.t); every solver runs inflate_cycles x {entropy, solve};
no partial: spread and entropy over every target coordinate (a Pose2 target: the compose form, heading included).
  direction 0 (fixed pose [3][N] -> landmark [2][N]):  keep the distance, turn to the bearing:  t <- p.t + ‖t − p.t‖ (cos, sin)(θp + b);
                                                         t == p.t stays.
  direction 1 (fixed landmark [2][N] -> pose [3][N]):  keep the translation, turn the heading:  θ <- wrap(atan2(l − t) − b);
                                                         t == l gives θ = wrap(−b).
CLOSED_FORM / NEWTON take that step once per cycle; GAUSS_NEWTON iterates it, the residual evaluated at every iterate until |r| <= tol;
NELDER_MEAD minimises r² over all target coordinates.  The direction is read from the block shapes."""
import math

import numpy as np

import oracle as ro

CLOSED_FORM, NEWTON, NELDER_MEAD, GAUSS_NEWTON = 0, 1, 2, 3


def wrap(a):
    return math.remainder(a, 2.0 * math.pi)


def measurement(mu, sigma, xi):
    """b = μ + σξ; σ < 0: Uniform(μ − |σ|, μ + |σ|) through the normal CDF of ξ"""
    if sigma >= 0.0:
        return mu + sigma * xi
    return mu - sigma * (math.erfc(-xi * 0.70710678118654752440) - 1.0)


def frechet_std(blk):
    """IIF calcStdBasicSpread: root of the summed coordinate variances, "no std yet -> 1" """
    _, sd = ro.belief_spread(blk)
    v = math.sqrt(float(np.sum(sd * sd)))
    return v if v > 1e-10 else 1.0


def residual(b, pose, lm):
    """rows: b (n,), pose (n, 3), lm (n, 2) -> (n,), the oracle's bearing-range residual, component 0"""
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    z = np.stack([b, np.zeros_like(b)], axis=1)
    return ro.residual_pose2point2br(z, np.atleast_2d(pose), np.atleast_2d(lm))[:, 0]


def _r(b, fx, t):
    """the residual of one particle, fixed block column fx and target point t (direction from the sizes)"""
    pose, lm = (fx, t) if len(t) == 2 else (t, fx)
    return float(residual([b], [pose], [lm])[0])


def step(b, fx, t):
    """the one-step rule of either direction -> the new target point"""
    t = np.array(t, dtype=np.float64)
    if t.size == 2:
        n = math.hypot(t[0] - fx[0], t[1] - fx[1])
        if n == 0.0:
            return t
        a = fx[2] + b
        return np.array([fx[0] + n * math.cos(a), fx[1] + n * math.sin(a)])
    dx, dy = fx[0] - t[0], fx[1] - t[1]
    psi = math.atan2(dy, dx) if (dx != 0.0 or dy != 0.0) else 0.0
    t[2] = wrap(psi - b)
    return t


def _uniforms(words):
    return [((w + 0.5) / 4294967296.0) for w in words]


def _add_entropy(t, spread, u):
    if t.size == 3:
        ex, ey, et = spread * (u[0] - 0.5), spread * (u[1] - 0.5), spread * (u[2] - 0.5)
        c, s = math.cos(t[2]), math.sin(t[2])
        t[0] += c * ex - s * ey
        t[1] += s * ex + c * ey
        t[2] = wrap(t[2] + et)
    else:
        t[0] += spread * (u[0] - 0.5)
        t[1] += spread * (u[1] - 0.5)


def conv_row(opts, mu, sigma, fixed, target, stream, solver, noise=None, noise_is_meas=False, nullhypo=0.0, spread_nh=3.0,
             tol=None, max_iters=None):
    """One convolution row.  fixed [df][N], target [dt][N] start points -> (out [dt][N], status [N]).
    `opts` is an oracle opts struct (N, seed, inflate_cycles, inflation are read from it); `stream` = stream_offset + row."""
    N = opts.n_particles
    seed = opts.seed
    cycles = max(1, opts.inflate_cycles)
    if tol is None:
        tol = 1e-8 if solver == NELDER_MEAD else 1e-12
    if max_iters is None:
        max_iters = 1000 if solver == NELDER_MEAD else 20
    dt = target.shape[0]
    out = np.array(target, dtype=np.float64, copy=True)
    if dt == 3:
        out[2] = [wrap(a) for a in out[2]]
    status = np.zeros(N, dtype=np.int32)
    b = np.empty(N)
    for i in range(N):
        xi = float(noise[i]) if noise is not None else float(ro.rng_normals(seed, stream, i, 1)[0])
        b[i] = xi if noise_is_meas else measurement(mu, sigma, xi)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    nullh = np.zeros(N, dtype=bool)
    nh_u = np.zeros((N, 3))
    nh_spread = 0.0
    if nullhypo > 0.0:
        nh_spread = spread_nh * frechet_std(out) if N > 1 else 0.0
        for i in range(N):
            w = ro.philox([i, stream & 0xFFFFFFFF, stream >> 32, 5 << 16], key)
            nullh[i] = _uniforms([w[0]])[0] < nullhypo
            nh_u[i] = _uniforms(w[1:4])
    for cyc in range(cycles):
        spread = opts.inflation * frechet_std(out) if (opts.inflation > 0.0 and N > 1) else 0.0
        for i in range(N):
            if nullh[i]:
                continue
            t = out[:, i].copy()
            fx = fixed[:, i]
            if spread > 0.0:
                _add_entropy(t, spread, ro.rng_entropy(seed, stream, i, cyc, dt))
            st = 0
            if solver in (CLOSED_FORM, NEWTON):
                t = step(b[i], fx, t)
            elif solver == GAUSS_NEWTON:
                st = 1
                for _ in range(max_iters):
                    if abs(_r(b[i], fx, t)) <= tol:
                        st = 0
                        break
                    t = step(b[i], fx, t)
            else:
                x, rc, _ = ro.nelder_mead(lambda x, bb=b[i], fx=fx: _r(bb, fx, x) ** 2, t, max_iters, tol)
                t = x
                if dt == 3:
                    t[2] = wrap(t[2])
                st = 1 if rc else 0
            out[:, i] = t
            status[i] = st
    if solver == NEWTON:
        for i in range(N):
            if not nullh[i]:
                status[i] = 0 if abs(_r(b[i], fixed[:, i], out[:, i])) <= tol else 1
    if solver == CLOSED_FORM:
        status[:] = 0
    if nh_spread > 0.0:
        for i in range(N):
            if nullh[i]:
                t = out[:, i].copy()
                _add_entropy(t, nh_spread, nh_u[i])
                out[:, i] = t
    return out, status


def conv(opts, mu, sigma, fixed, target, solver, noise=None, noise_is_meas=False, nullhypo=0.0, **kw):
    """C rows: mu / sigma [C], fixed [C][df][N], target [C][dt][N], noise [C][1][N] or None -> (out, status)"""
    C_ = len(mu)
    outs, sts = [], []
    for c in range(C_):
        o, s = conv_row(opts, float(mu[c]), float(sigma[c]), np.asarray(fixed[c]), np.asarray(target[c]), opts.stream_offset + c, solver,
                        None if noise is None else np.asarray(noise[c]).reshape(-1), noise_is_meas, nullhypo, **kw)
        outs.append(o)
        sts.append(s)
    return np.stack(outs), np.stack(sts)
