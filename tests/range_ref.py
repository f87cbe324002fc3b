"""Per-row restatement of the range-only factor convolutions (Point2Point2Range, Pose2Point2Range; RoME src/factors/Range2D.jl),
built only from the oracle's exported primitives: ro.rng_normals(..., 1), ro.rng_entropy, ro.belief_spread, ro.nelder_mead, ro.philox.
The loop is shaped after ro_conv_pose2point2br_mh (oracle/rome_oracle.c): measurement, start copy, nullhypo, cycles, solve.

Rules (include/rome_mi355.h): r = ρ − ‖t − a‖ with a = the fixed point / the fixed pose's translation; every solver runs
inflate_cycles x {entropy, solve}; a Pose2 target moves in (x, y) only (entropy in the compose form with a zero heading component);
CLOSED_FORM / NEWTON / GAUSS_NEWTON land on the radial projection (t == a leaves along +x, ρ <= 0 returns a)."""
import math

import numpy as np

import oracle as ro

CLOSED_FORM, NEWTON, NELDER_MEAD, GAUSS_NEWTON = 0, 1, 2, 3


def measurement(mu, sigma, xi):
    """ρ = μ + σξ; σ < 0: Uniform(μ − |σ|, μ + |σ|) through the normal CDF of ξ"""
    if sigma >= 0.0:
        return mu + sigma * xi
    return mu - sigma * (math.erfc(-xi * 0.70710678118654752440) - 1.0)


def frechet_std(blk):
    """IIF calcStdBasicSpread: root of the summed coordinate variances, "no std yet -> 1" """
    _, sd = ro.belief_spread(blk)
    v = math.sqrt(float(np.sum(sd * sd)))
    return v if v > 1e-10 else 1.0


def project(rho, a, t):
    """the radial projection of t onto the ring of radius ρ about a"""
    d = np.array([t[0] - a[0], t[1] - a[1]])
    n = math.hypot(d[0], d[1])
    if rho <= 0.0:
        return np.array([a[0], a[1]])
    if n == 0.0:
        return np.array([a[0] + rho, a[1]])
    return np.array([a[0] + rho * d[0] / n, a[1] + rho * d[1] / n])


def residual(rho, a, t):
    return rho - math.hypot(t[0] - a[0], t[1] - a[1])


def _uniforms(words):
    return [((w + 0.5) / 4294967296.0) for w in words]


def _add_entropy(t, spread, u):
    ex, ey = spread * (u[0] - 0.5), spread * (u[1] - 0.5)
    if t.size == 3:
        c, s = math.cos(t[2]), math.sin(t[2])
        t[0] += c * ex - s * ey
        t[1] += s * ex + c * ey
    else:
        t[0] += ex
        t[1] += ey


def conv_row(opts, mu, sigma, fixed, target, stream, solver, noise=None, noise_is_meas=False, nullhypo=0.0, spread_nh=3.0,
             tol=None, max_iters=None):
    """One convolution row.  fixed [df][N] (Point2 or Pose2 coordinates), target [dt][N] start points -> (out [dt][N], status [N]).
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
    status = np.zeros(N, dtype=np.int32)
    rho = np.empty(N)
    for i in range(N):
        xi = float(noise[i]) if noise is not None else float(ro.rng_normals(seed, stream, i, 1)[0])
        rho[i] = xi if noise_is_meas else measurement(mu, sigma, xi)
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
            a = fixed[:2, i]
            if spread > 0.0:
                _add_entropy(t, spread, ro.rng_entropy(seed, stream, i, cyc, dt))
            st = 0
            if solver in (CLOSED_FORM, NEWTON, GAUSS_NEWTON):
                t[:2] = project(rho[i], a, t)
            else:
                x, rc, _ = ro.nelder_mead(lambda x, r=rho[i], a=a: residual(r, a, x) ** 2, t[:2], max_iters, tol)
                t[:2] = x
                st = 1 if rc else 0
            out[:, i] = t
            status[i] = st
    if solver in (NEWTON, GAUSS_NEWTON):
        for i in range(N):
            if not nullh[i]:
                status[i] = 0 if (rho[i] > 0.0 and abs(residual(rho[i], fixed[:2, i], out[:, i])) <= tol) else 1
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
