// rome_conv_br.hpp -- the Pose2Point2BearingRange policy.  rome_conv_pose2.hip instantiates the convolution kernels and the fused sweep
// on it; the bearing-only policy PB<DIR> of rome_conv_range.hip takes its canonical form and its entropy from BR<DIR>.
#pragma once
#include "rome_conv.hpp"

namespace rome {

// ---- Pose2Point2BearingRange; DIR 0: pose fixed -> landmark target, DIR 1: landmark fixed -> pose target
template <int DIR>
struct BRCost {
  double b, rho; double fx[3];
  __device__ __forceinline__ double operator()(const double (&x)[DIR == 0 ? 2 : 3]) const {
    double r[2];
    if constexpr (DIR == 0) {
      const Se2 P = se2_from_coords(fx[0], fx[1], fx[2]);
      residual_bearingrange(b, rho, P, x[0], x[1], r);
    } else {
      const Se2 P = se2_from_coords(x[0], x[1], x[2]);
      residual_bearingrange(b, rho, P, fx[0], fx[1], r);
    }
    return r[0] * r[0] + r[1] * r[1];
  }
};

template <int DIR>
struct BR {
  static constexpr int DF = DIR == 0 ? 3 : 2, DT = DIR == 0 ? 2 : 3, DZ = 2, NL = 2, NK = 4;
  static constexpr int kHypoDir = DIR;  // multihypo over the landmark slot: DIR 0 target is fractional, DIR 1 fixed is fractional
  static constexpr bool kUniqueRoot = DIR == 0;   // pose direction: 2 equations / 3 unknowns, a ring of roots around the landmark
  struct Consts { double mu[2]; double sg[2]; };
  __device__ static __forceinline__ Consts load(const ConvArgs& a, int f, int) {
    Consts K; K.mu[0] = a.mu[2 * f]; K.mu[1] = a.mu[2 * f + 1]; K.sg[0] = a.L[2 * f]; K.sg[1] = a.L[2 * f + 1];
    return K;
  }
  __device__ static __forceinline__ Consts from_lds(const double* sk, int) {
    Consts K; K.mu[0] = sk[0]; K.mu[1] = sk[1]; K.sg[0] = sk[2]; K.sg[1] = sk[3];
    return K;
  }
  __device__ static __forceinline__ void measurement(const Consts& K, const double (&xi)[2], double (&z)[2]) {
    // rand(bearing), rand(range)  (BearingRange2D.jl:23).  sg >= 0: Normal(mu, sg).  sg < 0: Uniform(mu - |sg|, mu + |sg|)
    // (test/TestPoseAndPoint2Constraints.jl:95 uses Uniform(-π, π) bearings): the standard normal ξ is mapped through
    // its CDF, u = ½ erfc(-ξ/√2).
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (K.sg[k] >= 0.0) z[k] = K.mu[k] + K.sg[k] * xi[k];
      else z[k] = K.mu[k] - K.sg[k] * (erfc(-xi[k] * 0.70710678118654752440) - 1.0);
    }
  }
  // the (bearing, range) at which the residual vanishes on the pair (pose, landmark) (k_deconv; DIR 0 names the pair in that order):
  // atan2 and norm of pl = R(θp)ᵀ (l − p.t), in the expressions of residual_bearingrange.  l == p.t: (fast_atan2(0, 0), 0)
  __device__ static __forceinline__ void predict(const double (&p)[3], const double (&l)[2], double (&z)[2]) {
    const Se2 P = se2_from_coords(p[0], p[1], p[2]);
    const double dx = l[0] - P.x, dy = l[1] - P.y;
    const double plx = P.c * dx + P.s * dy;
    const double ply = P.c * dy - P.s * dx;
    z[0] = fast_atan2(ply, plx);
    z[1] = fast_sqrt(plx * plx + ply * ply);
  }
  __device__ static __forceinline__ void canonical(double (&t)[DT]) { if constexpr (DT == 3) t[2] = wrap_pi(t[2]); }
  // landmark direction: unique root, only the start-dependent solvers cycle; pose direction: every solver starts from the belief point
  __device__ static __forceinline__ bool needs_cycles(int solver, const Consts&) {
    return DIR == 1 || solver == kSolverNelderMead;   // (DIR 0 under GAUSS_NEWTON: unique root, see P2P2::needs_cycles)
  }
  struct Aux {};
  __device__ static __forceinline__ Aux init_aux(const double (&)[DT]) { return Aux{}; }
  __device__ static __forceinline__ void finalize(double (&)[DT], const Aux&) {}
  struct Ref { double c[DT]; };
  __device__ static __forceinline__ Ref make_ref(const double (&t0)[DT], const Aux&) {
    Ref r;
#pragma unroll
    for (int k = 0; k < DT; ++k) r.c[k] = t0[k];
    return r;
  }
  __device__ static __forceinline__ void tangent(const Ref& r, const double (&t)[DT], const Aux&, double (&d)[DT]) {
    d[0] = t[0] - r.c[0]; d[1] = t[1] - r.c[1];
    if constexpr (DT == 3) d[2] = wrap_pi(t[2] - r.c[2]);
  }
  template <int PPL>
  __device__ static __forceinline__ double spread(const double (&t)[PPL][DT], const Aux (&)[PPL], const bool (&act)[PPL], double inv, double den) {
    if constexpr (DT == 3) return spread_se2<PPL>(t, act, inv, den);
    else return spread_r2<PPL>(t, act, inv, den);
  }
  __device__ static __forceinline__ void add_entropy(double (&t)[DT], Aux&, double spread, const double (&u)[DT]) {
    if constexpr (DT == 3) {
      double s, c; fast_sincos(t[2], &s, &c);
      const double ex = spread * (u[0] - 0.5), ey = spread * (u[1] - 0.5), et = spread * (u[2] - 0.5);
      t[0] += c * ex - s * ey; t[1] += s * ex + c * ey; t[2] = wrap_pi(t[2] + et);
    } else { t[0] += spread * (u[0] - 0.5); t[1] += spread * (u[1] - 0.5); }
  }
  // Solver form of the residual (src/factors/BearingRange2D.jl:48-64): pl = R(θp)ᵀ (l − p.t) has norm n = ‖l − p.t‖ and angle
  // ψ − θp with ψ = atan2(l − p.t) the world bearing, so  r = ( sym_rem(b − (ψ − θp)), ρ − n )  without a sin/cos per evaluation
  // (same function as residual_bearingrange up to rounding; the residual entry points and GAUSS_NEWTON keep the literal form).
  //   DIR 0 (landmark): unique root  l* = p.t + ρ (cos, sin)(θp + b), prepared once (one sincos) -- CLOSED_FORM and NEWTON return it.
  //   DIR 1 (pose):     2 equations / 3 unknowns.  The block step keeps the ray landmark -> pose: move along it to the measured
  //                     range, then turn to the measured bearing (what the minimum-norm Gauss-Newton step approaches for ρ >> 1).
  struct Prep { double a0, a1; };
  __device__ static __forceinline__ Prep prepare(const Consts&, const double (&z)[2], const double (&fx)[DF]) {
    Prep P; P.a0 = 0.0; P.a1 = 0.0;
    if constexpr (DIR == 0) {
      double s, c; fast_sincos(fx[2] + z[0], &s, &c);
      P.a0 = fx[0] + z[1] * c; P.a1 = fx[1] + z[1] * s;
    }
    return P;
  }
  // the residual FUNCTOR itself at the target point t (pose fixed / landmark target, or the reverse)
  __device__ static __forceinline__ void functor(const double (&z)[2], const double (&fx)[DF], const double (&t)[DT], double (&r)[2]) {
    if constexpr (DIR == 0) residual_bearingrange(z[0], z[1], se2_from_coords(fx[0], fx[1], fx[2]), t[0], t[1], r);
    else residual_bearingrange(z[0], z[1], se2_from_coords(t[0], t[1], t[2]), fx[0], fx[1], r);
  }
  __device__ static __forceinline__ int verify(const Consts&, const double (&z)[2], const double (&fx)[DF], const double (&t)[DT], const Aux&, double tol) {
    double r[2]; functor(z, fx, t, r);
    return fmax(fabs(r[0]), fabs(r[1])) <= tol ? 0 : 1;
  }
  // Gauss-Newton on the functor (the oracle's br_newton): r = (sym_rem(b - atan2(pl)), rho - |pl|), pl = R(theta_p)^T (l - p.t), at every iterate;
  //   DIR 0: exact Newton step in the pose-frame polar chart of the landmark, (phi, n) += (r0, r1);  DIR 1: the block step along the ray.
  // Round 6 (as P2P2 / P3P3): an iterate is evaluated in the form its step needs.  The RANGE residual rho - |pl| comes first (one reciprocal
  // square root, shared with the step); the BEARING residual is evaluated only where the test max|r| <= tol can pass (wave-uniform: a
  // jittered start is never within 1e-12 of the measured range), and then as the angle of pl rotated by -b, whose small-angle branch
  // (-w_y / w_x for |w_y| < 1e-8 w_x: the verification iterate) needs no atan2.  The frame of the next iterate is carried: DIR 1 -- the
  // heading after the block step is (world bearing of the ray) - b, its (cos, sin) the unit ray rotated by -b: no sincos of the new
  // heading; DIR 0 -- phi + r0 = b (mod 2 pi) and n + r1 = rho, so the step lands on rho (cos b, sin b) in the fixed pose's frame: no atan2.
  // One sincos of the bearing sample per call; per cycle of the pose direction one atan2 (the heading itself, which the spread statistic and
  // the output need) instead of three and no sincos instead of two (k_conv<BR<1>, 3>: profiles/r06_other_factors_trace.md).
  __device__ static __forceinline__ int gauss_newton(const double (&z)[2], const double (&fx)[DF], double (&t)[DT], int max_iters, double tol) {
    double sz, cz; fast_sincos(z[0], &sz, &cz);
    double s = 0.0, c = 1.0;                                   // the frame the residual is taken in: the fixed pose (DIR 0) / the iterate (DIR 1)
    if constexpr (DIR == 0) fast_sincos(fx[2], &s, &c);
    bool fresh = true;                                         // DIR 1: (c, s) of the iterate's heading not carried yet (the start point)
    for (int it = 0; it < max_iters; ++it) {
      // landmark - pose translation in the world frame, its squared norm and 1 / norm
      const double dx = DIR == 0 ? t[0] - fx[0] : fx[0] - t[0], dy = DIR == 0 ? t[1] - fx[1] : fx[1] - t[1];
      const double n2 = dx * dx + dy * dy;
      double y = __builtin_amdgcn_rsq(n2);
      y = y * __builtin_fma(-0.5 * n2 * y, y, 1.5);
      y = y * __builtin_fma(-0.5 * n2 * y, y, 1.5);
      const bool ok = n2 > 0.0;
      const double r1 = z[1] - (ok ? n2 * y : 0.0);
      if (__builtin_amdgcn_ballot_w64(fabs(r1) <= tol) != 0) {   // somebody may be at a root: the bearing residual
        if constexpr (DIR == 1) { if (fresh) fast_sincos(t[2], &s, &c); }
        const double plx = c * dx + s * dy, ply = c * dy - s * dx;
        const double wx = plx * cz + ply * sz, wy = ply * cz - plx * sz;     // pl rotated by -b: its angle is -(b - atan2(pl))
        const bool small = wx > 0.0 && fabs(wy) < 1e-8 * wx;
        double r0;
        if (__builtin_amdgcn_ballot_w64(!small) == 0) r0 = -wy * fast_rcp(wx);
        else r0 = small ? -wy * fast_rcp(wx) : sym_rem(z[0] - fast_atan2(ply, plx));
        if (fmax(fabs(r0), fabs(r1)) <= tol) return 0;
      }
      if constexpr (DIR == 0) {       // (phi, n) += (r0, r1) = (b, rho) in the pose frame
        const double qx = z[1] * cz, qy = z[1] * sz;
        t[0] = fx[0] + c * qx - s * qy; t[1] = fx[1] + s * qx + c * qy;
      } else {                        // the block step along the ray (ring_step), the new heading's (cos, sin) = the unit ray rotated by -b
        const double k = ok ? z[1] * y : 0.0;
        t[0] = ok ? fx[0] - k * dx : fx[0] - z[1]; t[1] = fx[1] - k * dy;
        if constexpr (DT == 3) t[2] = (ok ? fast_atan2(dy, dx) : 0.0) - z[0];
        const double ux = ok ? dx * y : 1.0, uy = ok ? dy * y : 0.0;
        c = ux * cz + uy * sz; s = uy * cz - ux * sz;
        fresh = false;
      }
    }
    return 1;
  }
  // pose direction: move along the ray landmark -> pose to the measured range, then turn to the measured bearing.  One reciprocal
  // square root (v_rsq_f64 + two Newton steps) serves the unit vector; the world bearing is atan2 of the ray itself.
  __device__ static __forceinline__ void ring_step(const double (&z)[2], const double (&fx)[DF], double (&t)[DT]) {
    const double dx = fx[0] - t[0], dy = fx[1] - t[1];
    const double n2 = dx * dx + dy * dy;
    double y = __builtin_amdgcn_rsq(n2);
    y = y * __builtin_fma(-0.5 * n2 * y, y, 1.5);
    y = y * __builtin_fma(-0.5 * n2 * y, y, 1.5);
    const bool ok = n2 > 0.0;                                   // pose on the landmark: leave along +x
    const double k = ok ? z[1] * y : 0.0;
    t[0] = ok ? fx[0] - k * dx : fx[0] - z[1]; t[1] = fx[1] - k * dy;
    if constexpr (DT == 3) t[2] = (ok ? fast_atan2(dy, dx) : 0.0) - z[0];
  }
  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts&, const Prep& P, const double (&z)[2], const double (&fx)[DF],
                                              double (&t)[DT], Aux&, int max_iters, double tol) {
    int st = 0;
    if constexpr (DIR == 0 && (SOLVER == kSolverClosedForm || SOLVER == kSolverNewton)) { t[0] = P.a0; t[1] = P.a1; return 0; }
    else if constexpr (SOLVER == kSolverClosedForm) {
      ring_step(z, fx, t);
    } else if constexpr (SOLVER == kSolverNewton) {
      // pose direction: the block step from ANY start lands exactly on the member of the ring of roots that the start selects (the
      // closed form above IS that step); the residual there is evaluated only for the status array (verify_ring, after the last cycle)
      ring_step(z, fx, t);
    } else if constexpr (SOLVER == kSolverGaussNewton) {
      st = gauss_newton(z, fx, t, max_iters, tol);
    } else {
      BRCost<DIR> cost{z[0], z[1], {fx[0], fx[1], DF == 3 ? fx[DF - 1] : 0.0}};
      st = nelder_mead<DT>(cost, t, max_iters, tol);
    }
    if constexpr (DT == 3) t[2] = wrap_pi(t[2]);
    return st;
  }
};

}  // namespace rome
