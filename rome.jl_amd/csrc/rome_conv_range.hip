// rome_conv_range.hip -- the one-equation factors on the kernels of rome_conv.hpp: Point2Point2Range, Pose2Point2Range and
// Pose2Point2Bearing.  A ring / ray of roots: the wave-per-row kernels only (k_conv, k_conv_big), every solver cycles.
#include "rome_conv_br.hpp"

namespace rome {

// ---- range-only factors (src/factors/Range2D.jl): Point2Point2Range over [xi::Point2, lm::Point2], r = ρ − ‖lm − xi‖ (:14-17);
// Pose2Point2Range over [x::Pose2, lm::Point2], r = ρ − ‖lm − x.t‖ (:51-54), partial = (1, 2) on the pose (:44).
// Every (factor, direction) has a RING of roots around the anchor a -- the fixed point, or the fixed pose's translation: the start
// point selects the member, so every solver runs the inflation cycles {entropy, solve} as BR<1> does.  The solve moves the target's
// translation t only; a Pose2 target's heading passes through unchanged (neither the solve nor the entropy touches it).
//   CLOSED_FORM / NEWTON: the radial projection  t ← a + ρ (t − a)/‖t − a‖  (also the exact minimum-norm Gauss-Newton step);
//                         t == a leaves along +x, ρ ≤ 0 returns a (the minimiser of (ρ − n)² over n ≥ 0 is n = 0).
//   GAUSS_NEWTON:         that step iterated, the functor evaluated at every iterate until |r| ≤ tol; status 1 for ρ ≤ 0, as NEWTON
//                         reports it (at ρ = 0 the anchor zeroes the functor, but it is the degenerate ring, not a root).
//   NELDER_MEAD:          nelder_mead<2> on r² over (x, y) (at fixed θ on a Pose2 target).
// The measurement ρ = μ + σξ (σ < 0: Uniform(μ − |σ|, μ + |σ|) through the normal CDF of ξ, as BR::measurement); one standard normal
// per particle from the particle's own Philox call (rng_normals<1>).
struct RangeCost {
  double rho, ax, ay;
  __device__ __forceinline__ double operator()(const double (&x)[2]) const {
    const double dx = x[0] - ax, dy = x[1] - ay;
    const double r = rho - fast_sqrt(dx * dx + dy * dy);
    return r * r;
  }
};
// the radial projection of t onto the ring of radius ρ about a, from one v_rsq_f64 + two Newton steps (fast_rsqrt; ‖t − a‖ itself:
// range_norm, rome_device_math.hpp); the two degenerate rows as selects: t == a (n2 == 0) leaves along +x, ρ ≤ 0 returns a.
__device__ __forceinline__ void range_project(double rho, double ax, double ay, double& tx, double& ty) {
  const double dx = tx - ax, dy = ty - ay;
  const double n2 = dx * dx + dy * dy;
  const double y = fast_rsqrt(n2);
  const bool ok = n2 > 0.0, pos = rho > 0.0;
  const double k = pos ? (ok ? rho * y : rho) : 0.0;      // t = a + k e
  const double ex = ok ? dx : 1.0, ey = ok ? dy : 0.0;   // (t == a: e = +x)
  tx = __builtin_fma(k, ex, ax);
  ty = __builtin_fma(k, ey, ay);
}
// DF / DT: dimensions of the fixed and the target variable (2 = Point2, 3 = Pose2 coordinates); the anchor is (fx[0], fx[1])
template <int DF_, int DT_>
struct RangeBase {
  static constexpr int DF = DF_, DT = DT_, DZ = 1, NL = 1, NK = 2;
  static constexpr int kHypoDir = -1;           // no multihypo (refused by the entry points); the direction column is read from rows4
  static constexpr bool kUniqueRoot = false;    // a ring of roots: k_conv / k_conv_big only, every solver cycles
  struct Consts { double mu, sg; };
  __device__ static __forceinline__ Consts load(const ConvArgs& a, int f, int) { Consts K; K.mu = a.mu[f]; K.sg = a.L[f]; return K; }
  __device__ static __forceinline__ void measurement(const Consts& K, const double (&xi)[1], double (&z)[1]) {
    if (K.sg >= 0.0) z[0] = K.mu + K.sg * xi[0];
    else z[0] = K.mu - K.sg * (erfc(-xi[0] * 0.70710678118654752440) - 1.0);
  }
  __device__ static __forceinline__ Consts from_lds(const double* sk, int) { Consts K; K.mu = sk[0]; K.sg = sk[1]; return K; }   // (k_deconv)
  // the range at which the residual vanishes on the pair (k_deconv): ‖lm − x‖, a pose's heading is not read
  __device__ static __forceinline__ void predict(const double (&x)[DF], const double (&lm)[DT], double (&z)[1]) {
    z[0] = range_norm(lm[0] - x[0], lm[1] - x[1]);
  }
  __device__ static __forceinline__ void canonical(double (&)[DT]) {}   // (a Pose2 target's heading is passed through bit for bit)
  __device__ static __forceinline__ bool needs_cycles(int, const Consts&) { return true; }
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
  // the spread over the WHOLE target variable (Pose2: heading included), entropy and solve on the partial coordinates only
  template <int PPL>
  __device__ static __forceinline__ double spread(const double (&t)[PPL][DT], const Aux (&)[PPL], const bool (&act)[PPL], double inv, double den) {
    if constexpr (DT == 3) return spread_se2<PPL>(t, act, inv, den);
    else return spread_r2<PPL>(t, act, inv, den);
  }
  // Point2: t += spread (u − ½); Pose2: the compose form with a zero heading component, t += R(θ) spread (u_x − ½, u_y − ½)
  __device__ static __forceinline__ void add_entropy(double (&t)[DT], Aux&, double spread, const double (&u)[DT]) {
    const double ex = spread * (u[0] - 0.5), ey = spread * (u[1] - 0.5);
    if constexpr (DT == 3) {
      double s, c; fast_sincos(t[2], &s, &c);
      t[0] += c * ex - s * ey; t[1] += s * ex + c * ey;
    } else { t[0] += ex; t[1] += ey; }
  }
  struct Prep {};
  __device__ static __forceinline__ Prep prepare(const Consts&, const double (&)[1], const double (&)[DF]) { return Prep{}; }
  // the residual functor r = ρ − ‖t − a‖ at the target point
  __device__ static __forceinline__ double functor(const double (&z)[1], const double (&fx)[DF], const double (&t)[DT]) {
    return z[0] - range_norm(t[0] - fx[0], t[1] - fx[1]);
  }
  // status of a returned point: |r| <= tol (ρ ≤ 0 returns the anchor, which is no root: status 1)
  __device__ static __forceinline__ int verify(const Consts&, const double (&z)[1], const double (&fx)[DF], const double (&t)[DT], const Aux&, double tol) {
    return (z[0] > 0.0 && fabs(functor(z, fx, t)) <= tol) ? 0 : 1;
  }
  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts&, const Prep&, const double (&z)[1], const double (&fx)[DF],
                                              double (&t)[DT], Aux&, int max_iters, double tol) {
    if constexpr (SOLVER == kSolverClosedForm || SOLVER == kSolverNewton) {
      range_project(z[0], fx[0], fx[1], t[0], t[1]);
      return 0;
    } else if constexpr (SOLVER == kSolverGaussNewton) {
      for (int it = 0; it < max_iters; ++it) {
        if (fabs(functor(z, fx, t)) <= tol) return z[0] > 0.0 ? 0 : 1;   // (ρ <= 0: the anchor is no root, as verify reports it)
        range_project(z[0], fx[0], fx[1], t[0], t[1]);
      }
      return 1;
    } else {
      RangeCost cost{z[0], fx[0], fx[1]};
      double x[2] = {t[0], t[1]};
      const int st = nelder_mead<2>(cost, x, max_iters, tol);
      t[0] = x[0]; t[1] = x[1];
      return st;
    }
  }
};
// Point2Point2Range: both directions in one table (dir from rows4.y / the dir column): r is symmetric in (xi, lm), so the direction
// only decides which block is fixed and which is the target -- the per-particle work is the same
struct P2R : RangeBase<2, 2> {};
// Pose2Point2Range  DIR 0: pose fixed (anchor = its translation) -> landmark target;  DIR 1: landmark fixed -> pose target (x, y)
template <int DIR>
struct PPR : RangeBase<DIR == 0 ? 3 : 2, DIR == 0 ? 2 : 3> {};

// ---- bearing-only factor (src/factors/Bearing2D.jl:23-32): Pose2Point2Bearing over [p::Pose2, l::Point2],
// r = sym_rem(b − atan2(pl)), pl = R(θp)ᵀ (l − p.t): the bearing row of BR<DIR> on its own.  One equation: neither direction has a
// unique root, so every solver runs the inflation cycles {entropy, solve} on k_conv / k_conv_big, entropy and spread over ALL target
// coordinates (no partial: the compose form of BR<1> on a pose target).
//   DIR 0 (pose fixed -> landmark; roots: the open ray from p.t in world direction θp + b)
//     CLOSED_FORM / NEWTON: keep the distance, turn to the measured bearing:  n = ‖t − p.t‖,  t ← p.t + n (cos, sin)(θp + b) -- the
//     exact step (φ, n) += (r, 0) in the pose-frame polar chart (BR<0>'s Gauss-Newton step without its range row).  One sincos per
//     particle per call (Prep), n from range_norm; no atan2.  t == p.t: n = 0, t is returned unchanged (no direction has a length).
//   DIR 1 (landmark fixed -> pose; 1 equation, 3 unknowns)
//     CLOSED_FORM / NEWTON: keep the translation, turn the heading:  θ ← wrap_pi(atan2(l − t) − b), (x, y) untouched -- what the
//     minimum-norm Gauss-Newton step tends to as ‖l − t‖ grows (∂r/∂θ = 1, ‖∂r/∂t‖ = 1/‖l − t‖).  One atan2 per particle per cycle.
//     t == l: atan2(0, 0) = 0, θ = wrap_pi(−b) (a select).
//   GAUSS_NEWTON: that step iterated, the functor (literal form) evaluated at every iterate until |r| ≤ tol.
//   NELDER_MEAD:  nelder_mead<DT> on r² over all target coordinates, the heading wrapped on return.
// The measurement, the start-point reference, the tangent and the spread are RangeBase's (one scalar belief, σ < 0: Uniform; one
// standard normal per particle from the particle's own Philox call); the entropy and the canonical form are BR<DIR>'s.
template <int DIR>
struct BearingCost {
  double b; double fx[3];
  __device__ __forceinline__ double operator()(const double (&x)[DIR == 0 ? 2 : 3]) const {
    double r;
    if constexpr (DIR == 0) r = residual_bearing(b, se2_from_coords(fx[0], fx[1], fx[2]), x[0], x[1]);
    else r = residual_bearing(b, se2_from_coords(x[0], x[1], x[2]), fx[0], fx[1]);
    return r * r;
  }
};
template <int DIR>
struct PB : RangeBase<DIR == 0 ? 3 : 2, DIR == 0 ? 2 : 3> {
  using Base = RangeBase<DIR == 0 ? 3 : 2, DIR == 0 ? 2 : 3>;
  using typename Base::Consts;
  using typename Base::Aux;
  static constexpr int DF = Base::DF, DT = Base::DT;
  // the bearing at which the residual vanishes on the pair (pose, landmark) (k_deconv): the bearing row of BR<0>::predict
  __device__ static __forceinline__ void predict(const double (&p)[3], const double (&l)[2], double (&z)[1]) {
    const Se2 P = se2_from_coords(p[0], p[1], p[2]);
    const double dx = l[0] - P.x, dy = l[1] - P.y;
    z[0] = fast_atan2(P.c * dy - P.s * dx, P.c * dx + P.s * dy);
  }
  __device__ static __forceinline__ void canonical(double (&t)[DT]) { BR<DIR>::canonical(t); }
  __device__ static __forceinline__ void add_entropy(double (&t)[DT], Aux&, double spread, const double (&u)[DT]) {
    typename BR<DIR>::Aux none;
    BR<DIR>::add_entropy(t, none, spread, u);
  }
  struct Prep { double c, s; };   // DIR 0: (cos, sin)(θp + b)
  __device__ static __forceinline__ Prep prepare(const Consts&, const double (&z)[1], const double (&fx)[DF]) {
    Prep P; P.c = 1.0; P.s = 0.0;
    if constexpr (DIR == 0) fast_sincos(fx[2] + z[0], &P.s, &P.c);
    return P;
  }
  // the residual FUNCTOR itself at the target point t (pose fixed / landmark target, or the reverse)
  __device__ static __forceinline__ double functor(const double (&z)[1], const double (&fx)[DF], const double (&t)[DT]) {
    if constexpr (DIR == 0) return residual_bearing(z[0], se2_from_coords(fx[0], fx[1], fx[2]), t[0], t[1]);
    else return residual_bearing(z[0], se2_from_coords(t[0], t[1], t[2]), fx[0], fx[1]);
  }
  __device__ static __forceinline__ int verify(const Consts&, const double (&z)[1], const double (&fx)[DF], const double (&t)[DT], const Aux&, double tol) {
    return fabs(functor(z, fx, t)) <= tol ? 0 : 1;
  }
  __device__ static __forceinline__ void step(const Prep& P, const double (&z)[1], const double (&fx)[DF], double (&t)[DT]) {
    if constexpr (DIR == 0) {
      const double n = range_norm(t[0] - fx[0], t[1] - fx[1]);       // (n == 0: fx + 0 (c, s) = t)
      t[0] = __builtin_fma(n, P.c, fx[0]); t[1] = __builtin_fma(n, P.s, fx[1]);
    } else {
      const double dx = fx[0] - t[0], dy = fx[1] - t[1];
      const bool ok = dx != 0.0 || dy != 0.0;
      t[2] = wrap_pi((ok ? fast_atan2(dy, dx) : 0.0) - z[0]);
    }
  }
  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts&, const Prep& P, const double (&z)[1], const double (&fx)[DF],
                                              double (&t)[DT], Aux&, int max_iters, double tol) {
    if constexpr (SOLVER == kSolverClosedForm || SOLVER == kSolverNewton) {
      step(P, z, fx, t);
      return 0;
    } else if constexpr (SOLVER == kSolverGaussNewton) {
      for (int it = 0; it < max_iters; ++it) {
        if (fabs(functor(z, fx, t)) <= tol) return 0;
        step(P, z, fx, t);
      }
      return 1;
    } else {
      BearingCost<DIR> cost{z[0], {fx[0], fx[1], DF == 3 ? fx[DF - 1] : 0.0}};
      const int st = nelder_mead<DT>(cost, t, max_iters, tol);
      if constexpr (DT == 3) t[2] = wrap_pi(t[2]);
      return st;
    }
  }
};

// the range factors' Nelder-Mead instantiations of k_conv are not capped at four waves / SIMD (NmMinWaves, rome_conv.hpp); PB keeps
// the primary template's value
template <> struct NmMinWaves<P2R> { static constexpr int value = ROME_MIN_WAVES; };
template <> struct NmMinWaves<PPR<0>> { static constexpr int value = ROME_MIN_WAVES; };
template <> struct NmMinWaves<PPR<1>> { static constexpr int value = ROME_MIN_WAVES; };

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
// range factors: a ring of roots (kUniqueRoot = false) -> k_conv (N <= 512) / k_conv_big (N <= 4096) only
hipError_t launch_conv_point2point2range(const ConvArgs& a, int solver, hipStream_t s) { return launch_solver<P2R>(a, solver, s); }
hipError_t launch_conv_pose2point2range(const ConvArgs& a, int solver, hipStream_t s) {
  return a.dir_all == 0 ? launch_solver<PPR<0>>(a, solver, s) : launch_solver<PPR<1>>(a, solver, s);
}
// bearing-only factor: a ray / a two-parameter family of roots (kUniqueRoot = false) -> k_conv / k_conv_big only
hipError_t launch_conv_pose2point2bearing(const ConvArgs& a, int solver, hipStream_t s) {
  return a.dir_all == 0 ? launch_solver<PB<0>>(a, solver, s) : launch_solver<PB<1>>(a, solver, s);
}
hipError_t launch_deconv_range(int family, const DeconvArgs& a, hipStream_t s) {
  if (family == kDeconvBearing) return launch_deconv_t<PB<0>>(a, s);
  if (family == kDeconvPoint2Point2Range) return launch_deconv_t<P2R>(a, s);
  if (family == kDeconvPose2Point2Range) return launch_deconv_t<PPR<0>>(a, s);
  return hipErrorInvalidValue;
}

}  // namespace rome
