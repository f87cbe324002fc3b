// rome_conv_pose2.hip -- the Pose2 / Point2 sweep families: Pose2Pose2 (+ PriorPose2 rows) and Pose2Point2BearingRange on the kernels of
// rome_conv.hpp, and the fused one-launch sweep over both.
#include "rome_conv_br.hpp"

namespace rome {

// ------------------------------------------------------------------------------------------
// factor policies
// ------------------------------------------------------------------------------------------
// Coordinate form of the Pose2Pose2 residual (same function as
// src/factors/Pose2D.jl:51-67 evaluated through exp/compose/log on points):
//   r(z; p, q) = ( p.t + R(θp) z_t - q.t ,  wrap(θp + zθ - θq) )
// dir 0 (solve q): q̂ = p ∘ exp(z) is constant -> r = (q̂.t - q.t, wrap(q̂θ - qθ)): no transcendental per evaluation.
// dir 1 (solve p): one sincos(θp) per evaluation.
struct P2P2Cost {
  double zx, zy, a0, a1, a2; int dir;  // dir0: a = q̂ (x,y,θ) ; dir1: a = (q.x, q.y, qθ - zθ)
  __device__ __forceinline__ double operator()(const double (&x)[3]) const {
    double r0, r1, r2;
    if (dir == 0) { r0 = a0 - x[0]; r1 = a1 - x[1]; r2 = wrap_pi(a2 - x[2]); }
    else {
      double s, c; fast_sincos(x[2], &s, &c);
      r0 = x[0] + c * zx - s * zy - a0; r1 = x[1] + s * zx + c * zy - a1; r2 = wrap_pi(x[2] - a2);
    }
    return r0 * r0 + r1 * r1 + r2 * r2;
  }
};

struct P2P2 {
  static constexpr int DF = 3, DT = 3, DZ = 3, NL = 6, NK = 9;
  static constexpr int kHypoDir = 2;   // multihypo over the SECOND pose of the factor: the fractional side follows the row's direction
                                       // (dir 0: the target is one of the candidates; dir 1: the fixed pose is drawn per particle)
  static constexpr bool kUniqueRoot = true;   // r(z; p, ·) = 0 has exactly one solution: the start point cannot reach the proposal
  struct Consts { double mu[3]; double L[6]; int dir; };
  __device__ static __forceinline__ Consts load(const ConvArgs& a, int f, int dr) {
    Consts K;
#pragma unroll
    for (int k = 0; k < 3; ++k) K.mu[k] = a.mu[3 * f + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) K.L[k] = a.L[6 * f + k];
    K.dir = dr;
    return K;
  }
  // the same constants from the block's LDS image [μ(3), L(6)] (k_conv_flat)
  __device__ static __forceinline__ Consts from_lds(const double* sk, int dr) {
    Consts K;
#pragma unroll
    for (int k = 0; k < 3; ++k) K.mu[k] = sk[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) K.L[k] = sk[3 + k];
    K.dir = dr;
    return K;
  }
  __device__ static __forceinline__ void measurement(const Consts& K, const double (&xi)[3], double (&z)[3]) {
    z[0] = K.mu[0] + K.L[0] * xi[0];
    z[1] = K.mu[1] + K.L[1] * xi[0] + K.L[2] * xi[1];
    z[2] = K.mu[2] + K.L[3] * xi[0] + K.L[4] * xi[1] + K.L[5] * xi[2];
  }
  // the measurement at which r(z; p, q) vanishes (k_deconv): z = vee(log(p⁻¹ ∘ q)) in the uncoupled chart the residual uses
  __device__ static __forceinline__ void predict(const double (&p)[3], const double (&q)[3], double (&z)[3]) {
    predict_se2(se2_from_coords(p[0], p[1], p[2]), se2_from_coords(q[0], q[1], q[2]), z);
  }
  __device__ static __forceinline__ void canonical(double (&t)[3]) { t[2] = wrap_pi(t[2]); }
  // do the inflation cycles (entropy + re-solve) apply?  Only to Nelder-Mead, whose answer (to its g_tol of 1e-8 on the simplex spread)
  // depends on where it starts.  CLOSED_FORM and NEWTON return the unique root directly; GAUSS_NEWTON iterates on the residual functor
  // from the belief point until max|r| <= tol (1e-12): the root is unique, so no start point -- jittered or not -- and no number of
  // cycles can move the converged answer by more than the solver tolerance, and the entropy / re-solve rounds are not run.
  __device__ static __forceinline__ bool needs_cycles(int solver, const Consts& K) {
    return solver == kSolverNelderMead && K.dir != kDirPrior;
  }
  struct Aux {};
  __device__ static __forceinline__ Aux init_aux(const double (&)[3]) { return Aux{}; }
  __device__ static __forceinline__ void finalize(double (&)[3], const Aux&) {}
  // tangent coordinates of a point about the belief's particle 0 (the spread statistic, chunk by chunk: k_conv_big)
  struct Ref { double c[3]; };
  __device__ static __forceinline__ Ref make_ref(const double (&t0)[3], const Aux&) { return Ref{{t0[0], t0[1], t0[2]}}; }
  __device__ static __forceinline__ void tangent(const Ref& r, const double (&t)[3], const Aux&, double (&d)[3]) {
    d[0] = t[0] - r.c[0]; d[1] = t[1] - r.c[1]; d[2] = wrap_pi(t[2] - r.c[2]);
  }
  template <int PPL>
  __device__ static __forceinline__ double spread(const double (&t)[PPL][3], const Aux (&)[PPL], const bool (&act)[PPL], double inv, double den) {
    return spread_se2<PPL>(t, act, inv, den);
  }
  __device__ static __forceinline__ void add_entropy(double (&t)[3], Aux&, double spread, const double (&u)[3]) {
    double s, c; fast_sincos(t[2], &s, &c);
    const double ex = spread * (u[0] - 0.5), ey = spread * (u[1] - 0.5), et = spread * (u[2] - 0.5);
    t[0] += c * ex - s * ey; t[1] += s * ex + c * ey; t[2] = wrap_pi(t[2] + et);
  }

  // The root of the residual  r(z; p, q) = ( p.t + R(θp) z_t - q.t , wrap(θp + zθ - θq) )  (SURVEY A.5), per particle, for both
  // directions in ONE branch-free form (the direction is a per-thread value in k_conv_flat, where a wave spans two table rows):
  //   dir 0 (solve q): a = p ∘ exp_ϵ(z) = (p.t + R(θp) z_t, θp + zθ)
  //   dir 1 (solve p): a = (q.t - R(θq - zθ) z_t, θq - zθ)
  //   prior row:       a = z   = dir 0 about the identity pose (R(0) z_t + 0 is exact)
  // Rounding is pinned by explicit fma (the packed sweep, the wave-per-row kernel and the per-factor entry points agree bit for bit).
  struct Prep { double a0, a1, a2; };
  __device__ static __forceinline__ Prep prepare(const Consts& K, const double (&z)[3], const double (&fxc)[3]) {
    const bool pr = K.dir == kDirPrior, back = K.dir == 1;
    const double f0 = pr ? 0.0 : fxc[0], f1 = pr ? 0.0 : fxc[1], f2 = pr ? 0.0 : fxc[2];
    const double sg = back ? -1.0 : 1.0;          // a = f ± (...) as one fma with an exact ±1 factor: the rounding of the sum / difference
    Prep P;
    P.a2 = __builtin_fma(sg, z[2], f2);
    const double thr = back ? P.a2 : f2;
    double s, c; fast_sincos(thr, &s, &c);
    const double vx = __builtin_fma(c, z[0], -(s * z[1])), vy = __builtin_fma(s, z[0], c * z[1]);
    P.a0 = __builtin_fma(sg, vx, f0);
    P.a1 = __builtin_fma(sg, vy, f1);
    return P;
  }
  // the residual FUNCTOR itself (src/factors/Pose2D.jl:51-67 / PriorPose2.jl:37-47, through points) at the target point t.
  // Fn = what does not change over the iterates of a root-find: the fixed point (or the prior's sample point) and sin/cos of z_θ
  struct Fn { Se2 F; double sz, cz; };
  __device__ static __forceinline__ Fn functor_setup(const Consts& K, const double (&z)[3], const double (&fxc)[3]) {
    Fn f;
    if (K.dir == kDirPrior) { f.F = se2_from_coords(z[0], z[1], z[2]); f.sz = 0.0; f.cz = 1.0; }
    else { f.F = se2_from_coords(fxc[0], fxc[1], fxc[2]); fast_sincos(z[2], &f.sz, &f.cz); }
    return f;
  }
  __device__ static __forceinline__ void functor(const Consts& K, const Fn& f, const double (&z)[3], const double (&t)[3], double (&r)[3],
                                                 double* st = nullptr, double* ct = nullptr) {
    const Se2 T = se2_from_coords(t[0], t[1], t[2]);
    if (st) { *st = T.s; *ct = T.c; }   // (the Gauss-Newton step of dir 1 needs R'(θ) at the same θ)
    if (K.dir == kDirPrior) residual_priorpose2(f.F, T, r);
    else if (K.dir == 0) residual_pose2pose2(z[0], z[1], f.cz, f.sz, f.F, T, r);
    else residual_pose2pose2(z[0], z[1], f.cz, f.sz, T, f.F, r);
  }
  // status of a directly returned root: max|r| of the functor there against tol
  __device__ static __forceinline__ int verify(const Consts& K, const double (&z)[3], const double (&fxc)[3], const double (&t)[3], const Aux&, double tol) {
    // ONE branch-free evaluation for the three row kinds (the packed sweep's waves span rows of both directions): the residual of
    // gauss_newton's predicted-pose form -- S = the pose the factor predicts for q (dir 1: from the returned p), G = q -- which is the
    // functor's residual up to the sign of both parts; |r_θ| <= tol is decided on the unit vector (U11, U21) itself when it is small
    const bool back = K.dir == 1, prior = K.dir == kDirPrior;
    const Fn f = functor_setup(K, z, fxc);
    const Se2 T = se2_from_coords(t[0], t[1], t[2]);
    const double zx = prior ? 0.0 : z[0], zy = prior ? 0.0 : z[1];
    const double Xx = back ? T.x : f.F.x, Xy = back ? T.y : f.F.y, Xc = back ? T.c : f.F.c, Xs = back ? T.s : f.F.s;
    const double Mx = Xx + Xc * zx - Xs * zy, My = Xy + Xs * zx + Xc * zy, Mc = Xc * f.cz - Xs * f.sz, Ms = Xs * f.cz + Xc * f.sz;
    const double Gx = back ? f.F.x : T.x, Gy = back ? f.F.y : T.y, Gc = back ? f.F.c : T.c, Gs = back ? f.F.s : T.s;
    const double U11 = Mc * Gc + Ms * Gs, U21 = Mc * Gs - Ms * Gc;
    const bool small = U11 > 0.0 && fabs(U21) < 1e-8;
    const double r2 = small ? U21 : fast_atan2(U21, U11);
    return fmax(fabs(Gx - Mx), fmax(fabs(Gy - My), fabs(r2))) <= tol ? 0 : 1;
  }
  // Gauss-Newton on the functor (the oracle's p2p2_newton): evaluate r at the current point, step on the group.
  // Round 6 (i): the iterate carries (cos θ, sin θ) -- the heading residual is atan2(U21, U11) of a UNIT vector (U11, U21) = (cos r_θ, sin r_θ),
  // so the heading update θ += r_θ is the rotation of (c, s) by (U11, U21): no sincos of the new iterate; the ANGLE r_θ (the accumulated
  // output heading) costs one atan2 on the first iterate, from the second on |r_θ| < 1e-8 and r_θ = U21 to 1e-24.
  // Round 6 (ii): ONE loop body for both directions (a wave of the packed sweep spans rows of both), as P3P3::gauss_newton: the iteration
  // lives in the PREDICTED pose of q -- dir 0 / prior: the state S is q itself, the target G = F ∘ exp(z); dir 1: S = p ∘ exp(z) of the
  // iterate p, G = the fixed q -- with r = (G.t − S.t, angle of R_Sᵀ R_G) (dir 1: the functor's residual with both signs flipped; the
  // test is on max|r|) and the exact group update S.t += r_t, R_S ← R_S R(r_θ).  The oracle's dir-1 step linearises the translation
  // (J13, J23) and needs a third evaluation whenever the heading moved; this one lands on the root from any start: two evaluations.
  __device__ static __forceinline__ int gauss_newton(const Consts& K, const double (&z)[3], const double (&fxc)[3], double (&t)[3], int max_iters, double tol) {
    const bool back = K.dir == 1, prior = K.dir == kDirPrior;
    const Fn f = functor_setup(K, z, fxc);                     // (prior row: F = the sample point, z's rotation the identity)
    const Se2 T = se2_from_coords(t[0], t[1], t[2]);
    const double zx = prior ? 0.0 : z[0], zy = prior ? 0.0 : z[1];
    // M = X ∘ exp(z), X = the fixed pose (dir 0: the target is predicted from it) or the start iterate (dir 1: the state is)
    const double Xx = back ? T.x : f.F.x, Xy = back ? T.y : f.F.y, Xc = back ? T.c : f.F.c, Xs = back ? T.s : f.F.s;
    const double Mx = Xx + Xc * zx - Xs * zy, My = Xy + Xs * zx + Xc * zy, Mc = Xc * f.cz - Xs * f.sz, Ms = Xs * f.cz + Xc * f.sz;
    double Sx = back ? Mx : T.x, Sy = back ? My : T.y, Sc = back ? Mc : T.c, Ss = back ? Ms : T.s;
    const double Gx = back ? f.F.x : Mx, Gy = back ? f.F.y : My, Gc = back ? f.F.c : Mc, Gs = back ? f.F.s : Ms;
    double ang = back ? t[2] + z[2] : t[2];                    // the state's heading as an angle (the output accumulates the steps)
    int st = 1;
    for (int it = 0; it < max_iters; ++it) {
      const double U11 = Sc * Gc + Ss * Gs, U21 = Sc * Gs - Ss * Gc;
      const double r0 = Gx - Sx, r1 = Gy - Sy;
      const bool small = U11 > 0.0 && fabs(U21) < 1e-8;
      const double r2 = small ? U21 : fast_atan2(U21, U11);
      if (fmax(fabs(r0), fmax(fabs(r1), fabs(r2))) <= tol) { st = 0; break; }
      const double c0 = Sc, s0 = Ss;
      Sx += r0; Sy += r1; ang += r2;
      Sc = c0 * U11 - s0 * U21; Ss = s0 * U11 + c0 * U21;       // rotation by +r_θ
    }
    // the iterate itself: dir 0 / prior S; dir 1  R_p = R_S R(z_θ)ᵀ, p.t = S.t − R_p z_t, θ_p = θ_S − z_θ
    const double Pc = Sc * f.cz + Ss * f.sz, Ps = Ss * f.cz - Sc * f.sz;
    t[0] = back ? Sx - (Pc * zx - Ps * zy) : Sx;
    t[1] = back ? Sy - (Ps * zx + Pc * zy) : Sy;
    t[2] = back ? ang - z[2] : ang;
    return st;
  }

  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts& K, const Prep& P, const double (&z)[3], const double (&fxc)[3],
                                              double (&t)[3], Aux&, int max_iters, double tol) {
    int st = 0;
    if (K.dir == kDirPrior || SOLVER == kSolverClosedForm || SOLVER == kSolverNewton) {
      // PriorPose2 row: the sample exp_ϵ(hat(μ + Lξ)) itself is the proposal; relative rows: the unique root
      t[0] = P.a0; t[1] = P.a1; t[2] = wrap_pi(P.a2);
      return 0;
    }
    if constexpr (SOLVER == kSolverGaussNewton) st = gauss_newton(K, z, fxc, t, max_iters, tol);
    else {
      P2P2Cost cost{z[0], z[1], 0.0, 0.0, 0.0, K.dir};
      if (K.dir == 0) { cost.a0 = P.a0; cost.a1 = P.a1; cost.a2 = P.a2; }
      else { cost.a0 = fxc[0]; cost.a1 = fxc[1]; cost.a2 = P.a2; }
      st = nelder_mead<3>(cost, t, max_iters, tol);
    }
    t[2] = wrap_pi(t[2]);
    return st;
  }
};

// ------------------------------------------------------------------------------------------
// k_sweep_fused -- ONE launch for the whole sweep of a Pose2 / Point2 graph (MIT- / beehive-shaped: odometry + bearing-range
// sightings): the block range selects the family -- [bearing-range -> pose rows, one wavefront each | Pose2Pose2 + PriorPose2 rows,
// packed | bearing-range -> landmark rows, packed] -- and runs the SAME body as the family's own kernel (bit-identical proposals).
// A sub-generation table (a few thousand sightings) does not fill the chip and pays a launch each; fused, the long bearing-range ->
// pose waves are dispatched first and the packed blocks fill the machine around them.  CLOSED_FORM / NEWTON without status, plain
// rows (no pre-sampled noise / multihypo / nullhypo), 64 < N <= 128; anything else takes the per-family launches.
// ------------------------------------------------------------------------------------------
struct FusedArgs {
  ConvArgs br1, p2p2, br0;
  int nb_br1, nb_p2p2, nb_br0;       // blocks per part (each a multiple of 8: block b runs on XCD b % 8)
  int H, CPB2, CPB0;                 // packed parts: pair-threads per row, rows per block
  uint32_t magic;
};
// SOLVER: kSolverClosedForm (CLOSED_FORM / NEWTON) or kSolverGaussNewton -- the functor-iterating root-find of all three families in ONE
// launch (round 5: as three launches the bearing-range tables of an MIT-shaped graph are sub-generation, VALU-busy 0.30 / 0.39)
template <bool VEC2, int SOLVER>
__global__ void __launch_bounds__(256) k_sweep_fused(const FusedArgs f) {
  __shared__ double s_K[kFlatMaxRows * (FlatStage<P2P2>::kLanes + 2)];
  const int b = blockIdx.x;
  if (b < f.nb_br1) conv_wave_body<BR<1>, SOLVER, 2, true>(f.br1, xcd_contiguous_block(b, f.nb_br1));
  else if (b < f.nb_br1 + f.nb_p2p2) conv_flat_body<P2P2, SOLVER, false, VEC2, 1>(f.p2p2, f.H, f.CPB2, f.magic, xcd_contiguous_block(b - f.nb_br1, f.nb_p2p2), s_K);
  else conv_flat_body<BR<0>, SOLVER, false, VEC2, 1>(f.br0, f.H, f.CPB0, f.magic, xcd_contiguous_block(b - f.nb_br1 - f.nb_p2p2, f.nb_br0), s_K);
}

// The same with `multihypo` / `nullhypo` columns on the bearing-range tables (the beehive of BASELINE configs[3]: ambiguous re-sightings,
// test/testMultimodalRangeBearing.jl:53): both sighting directions run the feature-complete wave-per-row body (the fractional
// hypotheses need statistics over a row's particles), the odometry table stays packed.  One launch instead of three for a graph whose
// tables are all sub-generation; bit-identical to the per-family launches.
template <bool VEC2>
__global__ void __launch_bounds__(256) k_sweep_fused_mh(const FusedArgs f) {
  __shared__ double s_K[kFlatMaxRows * (FlatStage<P2P2>::kLanes + 2)];
  const int b = blockIdx.x;
  if (b < f.nb_br1) conv_wave_body<BR<1>, kSolverClosedForm, 2, false>(f.br1, xcd_contiguous_block(b, f.nb_br1));
  else if (b < f.nb_br1 + f.nb_p2p2) conv_flat_body<P2P2, kSolverClosedForm, false, VEC2, 1>(f.p2p2, f.H, f.CPB2, f.magic, xcd_contiguous_block(b - f.nb_br1, f.nb_p2p2), s_K);
  else conv_wave_body<BR<0>, kSolverClosedForm, 2, false>(f.br0, xcd_contiguous_block(b - f.nb_br1 - f.nb_p2p2, f.nb_br0));
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
hipError_t launch_conv_pose2pose2(const ConvArgs& a, int solver, hipStream_t s) { return launch_solver<P2P2>(a, solver, s); }
hipError_t launch_conv_bearingrange(const ConvArgs& a, int solver, hipStream_t s) {
  return a.dir_all == 0 ? launch_solver<BR<0>>(a, solver, s) : launch_solver<BR<1>>(a, solver, s);
}
static bool plain_rows(const ConvArgs& a) { return a.rows4 && !a.noise && !a.alt_var && !a.nullhypo && !a.status && !a.row_stream && !a.meas_block; }
static bool hypo_rows(const ConvArgs& a) { return a.rows4 && !a.noise && !a.status && !a.row_stream && !a.meas_block && (a.alt_var || a.nullhypo); }
// the whole sweep of a Pose2 / Point2 graph: fused into one launch when every family takes its plain kernel, else family by family
hipError_t launch_sweep_pose2(const ConvArgs* p2p2, const ConvArgs* br1, const ConvArgs* br0, int solver, hipStream_t s) {
  const int N = p2p2 ? p2p2->N : (br1 ? br1->N : (br0 ? br0->N : 0));
  const bool shape_ok = p2p2 && br1 && br0 && p2p2->n_conv > 0 && br1->n_conv > 0 && br0->n_conv > 0 &&
                        (solver == kSolverClosedForm || solver == kSolverNewton || solver == kSolverGaussNewton) && N > 64 && N <= 128 && br1->N == N && br0->N == N &&
                        br1->dir_all == 1 && br0->dir_all == 0;
  // sighting tables with multihypo / nullhypo columns: the fused launch with the feature-complete wave bodies for both directions
  const bool fusable_mh = shape_ok && solver != kSolverGaussNewton && plain_rows(*p2p2) && (hypo_rows(*br1) || plain_rows(*br1)) && (hypo_rows(*br0) || plain_rows(*br0)) &&
                          (hypo_rows(*br1) || hypo_rows(*br0));
  const bool fusable = shape_ok &&
                       plain_rows(*p2p2) && plain_rows(*br1) && plain_rows(*br0) &&
                       // the fused kernel runs every part at the register allocation of the bearing-range pose body (88 VGPRs, 5 waves
                       // per SIMD instead of the packed sweep's 8): worth two saved launches unless the odometry table is both huge and
                       // dominant
                       (p2p2->n_conv <= 100000 || 10 * (br1->n_conv + br0->n_conv) >= p2p2->n_conv);
  if (!fusable && !fusable_mh) {
    hipError_t e = hipSuccess;
    if (br1 && br1->n_conv > 0 && (e = launch_conv_bearingrange(*br1, solver, s)) != hipSuccess) return e;
    if (p2p2 && p2p2->n_conv > 0 && (e = launch_conv_pose2pose2(*p2p2, solver, s)) != hipSuccess) return e;
    if (br0 && br0->n_conv > 0 && (e = launch_conv_bearingrange(*br0, solver, s)) != hipSuccess) return e;
    return e;
  }
  FusedArgs f;
  f.br1 = *br1; f.p2p2 = *p2p2; f.br0 = *br0;
  f.H = (N + 1) / 2;
  const int cpb = kFlatThreads / f.H;
  f.CPB2 = cpb < kFlatMaxRows ? cpb : kFlatMaxRows; f.CPB0 = f.CPB2;
  f.magic = (65536u + (uint32_t)f.H - 1u) / (uint32_t)f.H;
  for (int t = 0; t < kFlatThreads; ++t) if ((int)(((uint32_t)t * f.magic) >> 16) != t / f.H) return hipErrorInvalidValue;
  auto up8 = [](int n) { return (n + 7) & ~7; };
  f.nb_br1 = up8((br1->n_conv + ROME_WPB - 1) / ROME_WPB);
  f.nb_p2p2 = up8((p2p2->n_conv + f.CPB2 - 1) / f.CPB2);
  f.nb_br0 = fusable_mh ? up8((br0->n_conv + ROME_WPB - 1) / ROME_WPB) : up8((br0->n_conv + f.CPB0 - 1) / f.CPB0);
  const uintptr_t al = (uintptr_t)p2p2->bel_fixed | (uintptr_t)p2p2->out | (uintptr_t)p2p2->mirror_out | (uintptr_t)br0->bel_fixed |
                       (uintptr_t)br0->out | (uintptr_t)br0->mirror_out;
  const bool vec2 = (N % 2 == 0) && (al % 16 == 0);
  const int nb = f.nb_br1 + f.nb_p2p2 + f.nb_br0;
  if (fusable_mh) {
    if (vec2) hipLaunchKernelGGL((k_sweep_fused_mh<true>), dim3(nb), dim3(256), 0, s, f);
    else      hipLaunchKernelGGL((k_sweep_fused_mh<false>), dim3(nb), dim3(256), 0, s, f);
  } else if (solver == kSolverGaussNewton) {
    if (vec2) hipLaunchKernelGGL((k_sweep_fused<true, kSolverGaussNewton>), dim3(nb), dim3(256), 0, s, f);
    else      hipLaunchKernelGGL((k_sweep_fused<false, kSolverGaussNewton>), dim3(nb), dim3(256), 0, s, f);
  } else {
    if (vec2) hipLaunchKernelGGL((k_sweep_fused<true, kSolverClosedForm>), dim3(nb), dim3(256), 0, s, f);
    else      hipLaunchKernelGGL((k_sweep_fused<false, kSolverClosedForm>), dim3(nb), dim3(256), 0, s, f);
  }
  return hipGetLastError();
}
// approxDeconv of the two families of this unit (k_deconv, rome_conv.hpp)
hipError_t launch_deconv_pose2(int family, const DeconvArgs& a, hipStream_t s) {
  if (family == kDeconvPose2Pose2) return launch_deconv_t<P2P2>(a, s);
  if (family == kDeconvBearingRange) return launch_deconv_t<BR<0>>(a, s);
  return hipErrorInvalidValue;
}

}  // namespace rome
