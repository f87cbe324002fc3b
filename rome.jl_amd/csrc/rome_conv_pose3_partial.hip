// rome_conv_pose3_partial.hip -- the partial Pose3 factors (src/factors/PartialPose3.jl) on the kernels of rome_conv.hpp:
// Pose3Pose3XYYaw, partial = (1, 2, 6), PriorPose3ZRP, partial = (3, 4, 5), and Pose3Pose3Rotation, partial = (4, 5, 6).  The partial rule of DESIGN §12a on a Pose3 target: the
// spread over the whole variable (P3P3::spread, all six tangent coordinates), entropy and solve on the partial coordinates only, every
// other coordinate stored from the loaded value -- bit for bit.  The policies stay off the packed sweep (kUniqueRoot = false): it has no
// partial notion.  The wave-per-row kernels only (k_conv, k_conv_big).
#include "rome_conv_p3.hpp"

namespace rome {

// What the policies share.  The state is the COORDINATES (t, ω) from load to store (no Aux, no Log on the way out); a quaternion is
// built only where the statistic over all six coordinates needs one.  I0, I1, I2: the partial coordinates (0-based).
// The entropy is ADDITIVE on the partial coordinates, t[I] += spread (u[I] − ½): the compose form u0 ∘ exp(e) of P3P3::add_entropy would move
// the other three as soon as the pose is tilted.  Uniforms: the d = 6 draw, three of them used.
template <int I0, int I1, int I2>
struct P3Partial {
  static constexpr int DF = 6, DT = 6, DZ = 3;
  static constexpr int kHypoDir = -1;          // no multihypo (refused by the entry points)
  static constexpr bool kUniqueRoot = false;   // never the packed sweep
  __device__ static __forceinline__ void canonical(double (&)[6]) {}
  struct Aux {};
  __device__ static __forceinline__ Aux init_aux(const double (&)[6]) { return Aux{}; }
  __device__ static __forceinline__ void finalize(double (&)[6], const Aux&) {}
  using Ref = P3P3::Ref;
  __device__ static __forceinline__ Ref make_ref(const double (&t0)[6], const Aux&) { return P3P3::make_ref(t0, P3P3::init_aux(t0)); }
  __device__ static __forceinline__ void tangent(const Ref& r, const double (&t)[6], const Aux&, double (&d)[6]) {
    P3P3::tangent(r, t, P3P3::init_aux(t), d);
  }
  template <int PPL>
  __device__ static __forceinline__ double spread(const double (&t)[PPL][6], const Aux (&)[PPL], const bool (&act)[PPL], double inv, double den) {
    P3P3::Aux A[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) A[k] = P3P3::init_aux(t[k]);
    return P3P3::template spread<PPL>(t, A, act, inv, den);
  }
  __device__ static __forceinline__ void add_entropy(double (&t)[6], Aux&, double spread, const double (&u)[6]) {
    t[I0] += spread * (u[I0] - 0.5); t[I1] += spread * (u[I1] - 0.5); t[I2] += spread * (u[I2] - 0.5);
  }
};

// ---- Pose3Pose3XYYaw (PartialPose3.jl:101-136) over [p, q]: r = the Pose2Pose2 residual of (z, p₂, q₂), p₂ = (p.t_xy, ψ(R_p)) the SE(2)
// projection (rome_device_math.hpp).  Unknowns: the target's (x, y, ω_z); its z, ω_x, ω_y are constants of the solve.
// (ψ*, t*) = the heading and xy translation the factor predicts for the target:
//   dir 0 (solve q): ψ* = ψ_p + z_θ,  t* = p.t_xy + R₂(ψ_p) z_xy
//   dir 1 (solve p): ψ* = ψ_q − z_θ,  t* = q.t_xy − R₂(ψ_p) z_xy with ψ_p the yaw of the iterate itself
// xy is that closed form at every iterate; ω_z = s solves g(s) = wrap(ψ(Exp(ω_x, ω_y, s)) − ψ*) = 0 by Newton, ∂ψ/∂s = yaw_rate.
//   CLOSED_FORM / NEWTON: from s₀ = wrap(ψ*) (the principal branch; the start point's ω_z is not read), to |g| <= tol, at most max_iters steps.
//   GAUSS_NEWTON:         from the start particle's own ω_z, the functor evaluated at every iterate, to max|r| <= tol; one pass.
//   NELDER_MEAD:          nelder_mead<3> on Σr² over (x, y, ω_z); the only solver that runs the inflation cycles.
// A pose tilted so far that |∂ψ/∂s| < 1e-6 takes unit steps (no division by a vanishing rate); status 1 at the cap as everywhere.
struct XYYCost {
  double zx, zy, cz, sz; Se2 F; double wx, wy; int dir;
  __device__ __forceinline__ double operator()(const double (&x)[3]) const {
    double c[3], u[3], r[3];
    so3_col1_dz(wx, wy, x[2], c, u);
    const Se2 T = se2_of_pose3(x[0], x[1], c[0], c[1]);
    if (dir == 0) residual_pose3pose3xyyaw(zx, zy, cz, sz, F, T, r); else residual_pose3pose3xyyaw(zx, zy, cz, sz, T, F, r);
    return r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  }
};

struct P3XYY : P3Partial<0, 1, 5> {
  static constexpr int NL = 6, NK = 9;
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
  __device__ static __forceinline__ void measurement(const Consts& K, const double (&xi)[3], double (&z)[3]) {   // the d = 3 normal rule of P2P2
    z[0] = K.mu[0] + K.L[0] * xi[0];
    z[1] = K.mu[1] + K.L[1] * xi[0] + K.L[2] * xi[1];
    z[2] = K.mu[2] + K.L[3] * xi[0] + K.L[4] * xi[1] + K.L[5] * xi[2];
  }
  __device__ static __forceinline__ Consts from_lds(const double* sk, int dr) {   // (k_deconv)
    Consts K;
#pragma unroll
    for (int k = 0; k < 3; ++k) K.mu[k] = sk[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) K.L[k] = sk[3 + k];
    K.dir = dr;
    return K;
  }
  // the measurement at which the residual vanishes on the pair (k_deconv): the Pose2Pose2 measurement of the two SE(2) projections
  __device__ static __forceinline__ void predict(const double (&p)[6], const double (&q)[6], double (&z)[3]) {
    double cp[3], cq[3], u[3];
    so3_col1_dz(p[3], p[4], p[5], cp, u);
    so3_col1_dz(q[3], q[4], q[5], cq, u);
    predict_se2(se2_of_pose3(p[0], p[1], cp[0], cp[1]), se2_of_pose3(q[0], q[1], cq[0], cq[1]), z);
  }
  __device__ static __forceinline__ bool needs_cycles(int solver, const Consts&) { return solver == kSolverNelderMead; }
  // F = the fixed pose's projection; ψ*; a = t* (dir 0) or q.t_xy (dir 1: t* follows the iterate's own yaw)
  struct Prep { Se2 F; double psi, ax, ay; };
  __device__ static __forceinline__ Prep prepare(const Consts& K, const double (&z)[3], const double (&fxc)[6]) {
    Prep P;
    double c[3], u[3];
    so3_col1_dz(fxc[3], fxc[4], fxc[5], c, u);
    P.F = se2_of_pose3(fxc[0], fxc[1], c[0], c[1]);
    const double psiF = yaw_of_col1(c[0], c[1]);
    const bool back = K.dir != 0;
    P.psi = back ? psiF - z[2] : psiF + z[2];
    P.ax = back ? P.F.x : P.F.x + (P.F.c * z[0] - P.F.s * z[1]);
    P.ay = back ? P.F.y : P.F.y + (P.F.s * z[0] + P.F.c * z[1]);
    return P;
  }
  // the target at ω_z = s: its projection T (xy by the closed form), g(s) and ∂ψ/∂s
  struct Eval { Se2 T; double g, rate; };
  __device__ static __forceinline__ Eval eval(const Consts& K, const Prep& P, const double (&z)[3], double wx, double wy, double s) {
    double c[3], u[3];
    so3_col1_dz(wx, wy, s, c, u);
    Eval E;
    E.g = wrap_pi(yaw_of_col1(c[0], c[1]) - P.psi);
    E.rate = yaw_rate(c, u);
    E.T = se2_of_pose3(P.ax, P.ay, c[0], c[1]);
    if (K.dir != 0) {   // (wave-uniform)
      E.T.x = P.ax - (E.T.c * z[0] - E.T.s * z[1]);
      E.T.y = P.ay - (E.T.s * z[0] + E.T.c * z[1]);
    }
    return E;
  }
  // the residual FUNCTOR at the target's projection T
  __device__ static __forceinline__ double functor_max(const Consts& K, const Prep& P, const double (&z)[3], double cz, double sz, const Se2& T) {
    double r[3];
    if (K.dir == 0) residual_pose3pose3xyyaw(z[0], z[1], cz, sz, P.F, T, r); else residual_pose3pose3xyyaw(z[0], z[1], cz, sz, T, P.F, r);
    return fmax(fabs(r[0]), fmax(fabs(r[1]), fabs(r[2])));
  }
  __device__ static __forceinline__ int verify(const Consts& K, const double (&z)[3], const double (&fxc)[6], const double (&t)[6], const Aux&, double tol) {
    const Prep P = prepare(K, z, fxc);
    double c[3], u[3], sz, cz;
    so3_col1_dz(t[3], t[4], t[5], c, u);
    fast_sincos(z[2], &sz, &cz);
    return functor_max(K, P, z, cz, sz, se2_of_pose3(t[0], t[1], c[0], c[1])) <= tol ? 0 : 1;
  }
  // Newton on s from s0.  FUNCTOR: the convergence test is the functor at the iterate (GAUSS_NEWTON), else |g| <= tol.  The loop ends when
  // every lane of the wave has converged (a converged lane keeps its s); at the cap the xy of the last iterate is evaluated once more.
  template <bool FUNCTOR>
  __device__ static __forceinline__ int yaw_newton(const Consts& K, const Prep& P, const double (&z)[3], double (&t)[6], double s, int max_iters, double tol) {
    [[maybe_unused]] double sz = 0.0, cz = 1.0;
    if constexpr (FUNCTOR) fast_sincos(z[2], &sz, &cz);
    bool done = false;
    Eval E = eval(K, P, z, t[3], t[4], s);
    for (int it = 0; it < max_iters; ++it) {
      if (it > 0) E = eval(K, P, z, t[3], t[4], s);
      if constexpr (FUNCTOR) done = functor_max(K, P, z, cz, sz, E.T) <= tol;
      else done = fabs(E.g) <= tol;
      if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
      if (!done) s -= E.g / (fabs(E.rate) > 1e-6 ? E.rate : 1.0);
    }
    if (__builtin_amdgcn_ballot_w64(!done) != 0) {   // the cap: a lane that did not converge returns its last iterate, xy included
      const Eval E2 = eval(K, P, z, t[3], t[4], s);
      E.T.x = done ? E.T.x : E2.T.x; E.T.y = done ? E.T.y : E2.T.y;
    }
    t[0] = E.T.x; t[1] = E.T.y; t[5] = s;
    return done ? 0 : 1;
  }
  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts& K, const Prep& P, const double (&z)[3], const double (&)[6],
                                              double (&t)[6], Aux&, int max_iters, double tol) {
    if constexpr (SOLVER == kSolverClosedForm || SOLVER == kSolverNewton) return yaw_newton<false>(K, P, z, t, wrap_pi(P.psi), max_iters, tol);
    else if constexpr (SOLVER == kSolverGaussNewton) return yaw_newton<true>(K, P, z, t, t[5], max_iters, tol);
    else {
      XYYCost cost;
      cost.zx = z[0]; cost.zy = z[1]; fast_sincos(z[2], &cost.sz, &cost.cz);
      cost.F = P.F; cost.wx = t[3]; cost.wy = t[4]; cost.dir = K.dir;
      double x[3] = {t[0], t[1], t[5]};
      const int st = nelder_mead<3>(cost, x, max_iters, tol);
      t[0] = x[0]; t[1] = x[1]; t[5] = x[2];
      return st;
    }
  }
};

// ---- PriorPose3ZRP (PartialPose3.jl:12-46): z_s = μ_z + σ_z ξ₀, (r, p) = μ_rp + L_rp (ξ₁, ξ₂), R = R_y(p) R_x(r) (RotYX(p, r), :32) as the
// unit quaternion (c_p c_r, c_p s_r, s_p c_r, −s_p s_r) on half angles, ω = Log R; the sample is (z_s, ω_x, ω_y) -- ω_z is dropped (:41-45).
// L = [σ_z, packed 2x2 Cholesky of the roll / pitch covariance].  The proposal is the target's OWN particle with coordinates 3, 4, 5
// replaced: a prior row that reads the target belief (the table's fixed block is the target block; it is not read).  No iteration, no
// cycles: every solver returns the same thing, one instantiation per launch shape.
struct P3ZRP : P3Partial<2, 3, 4> {
  static constexpr int NL = 4, NK = 7;
  struct Consts { double mu[3]; double L[4]; };
  __device__ static __forceinline__ Consts load(const ConvArgs& a, int f, int) {
    Consts K;
#pragma unroll
    for (int k = 0; k < 3; ++k) K.mu[k] = a.mu[3 * f + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) K.L[k] = a.L[4 * f + k];
    return K;
  }
  __device__ static __forceinline__ void measurement(const Consts& K, const double (&xi)[3], double (&z)[3]) {
    const double r = K.mu[1] + K.L[1] * xi[1];
    const double p = K.mu[2] + K.L[2] * xi[1] + K.L[3] * xi[2];
    double sr, cr, sp, cp;
    fast_sincos(0.5 * r, &sr, &cr); fast_sincos(0.5 * p, &sp, &cp);
    const double q[4] = {cp * cr, cp * sr, sp * cr, -(sp * sr)};
    double w[3];
    quat_log(q, w);
    z[0] = K.mu[0] + K.L[0] * xi[0]; z[1] = w[0]; z[2] = w[1];
  }
  __device__ static __forceinline__ bool needs_cycles(int, const Consts&) { return false; }
  struct Prep {};
  __device__ static __forceinline__ Prep prepare(const Consts&, const double (&)[3], const double (&)[6]) { return Prep{}; }
  __device__ static __forceinline__ int verify(const Consts&, const double (&)[3], const double (&)[6], const double (&)[6], const Aux&, double) { return 0; }
  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts&, const Prep&, const double (&z)[3], const double (&)[6], double (&t)[6], Aux&, int, double) {
    t[2] = z[0]; t[3] = z[1]; t[4] = z[2];
    return 0;
  }
};

// ---- Pose3Pose3Rotation (PartialPose3.jl:204-227) over [p, q]: r = z − Log(R_pᵀ R_q), z a rotation vector, Log the principal one.
// Unknowns: the target's (ω_x, ω_y, ω_z); its translation is a constant of the solve (and no translation enters the residual).
// The root rotation qa, as a unit quaternion:
//   dir 0 (solve q): R_q = R_p Exp(z),   qa = q_p ⊗ q_z
//   dir 1 (solve p): R_p = R_q Exp(−z),  qa = q_q ⊗ conj(q_z)
// It is the zero of the functor whenever |z| < π; for |z| >= π the functor has none (z − Log(Exp z) is a whole turn about the axis), the
// closed form returns the same rotation and every status output reports the functor: status 1 there.
//   CLOSED_FORM / NEWTON: ω = Log qa (the start point's ω is not read).
//   GAUSS_NEWTON:         from the start particle's own rotation u: e = conj(qa) ⊗ u (= Exp(z)ᵀ R_pᵀ R_q for dir 0, the mirrored product for
//                         dir 1), u <- u ⊗ conj(e) -- the residual rotation itself is the update, as in P3P3::gauss_newton; the functor at
//                         every iterate, its Log taken only where the test can pass; one pass, the loop ends on a wave ballot.
//   NELDER_MEAD:          nelder_mead<3> on Σr² over (ω_x, ω_y, ω_z) through 3x3 frames (as P3P3Cost); the only solver that cycles.
struct ROTCost {
  double z[3]; double F[9]; int dir;   // F: the fixed pose's frame
  __device__ __forceinline__ double operator()(const double (&x)[3]) const {
    double T[9], r[3];
    so3_exp(x, T);
    if (dir == 0) residual_pose3pose3rotation(z, F, T, r); else residual_pose3pose3rotation(z, T, F, r);
    return r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  }
};

struct P3ROT : P3Partial<3, 4, 5> {
  static constexpr int NL = 6, NK = 9;
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
  __device__ static __forceinline__ void measurement(const Consts& K, const double (&xi)[3], double (&z)[3]) {   // the d = 3 normal rule of P3XYY
    z[0] = K.mu[0] + K.L[0] * xi[0];
    z[1] = K.mu[1] + K.L[1] * xi[0] + K.L[2] * xi[1];
    z[2] = K.mu[2] + K.L[3] * xi[0] + K.L[4] * xi[1] + K.L[5] * xi[2];
  }
  __device__ static __forceinline__ Consts from_lds(const double* sk, int dr) {   // (k_deconv)
    Consts K;
#pragma unroll
    for (int k = 0; k < 3; ++k) K.mu[k] = sk[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) K.L[k] = sk[3 + k];
    K.dir = dr;
    return K;
  }
  // the measurement at which the residual vanishes on the pair (k_deconv): Log(R_pᵀ R_q), the principal rotation vector
  __device__ static __forceinline__ void predict(const double (&p)[6], const double (&q)[6], double (&z)[3]) {
    double qp[4], qq[4], e[4];
    quat_exp(&p[3], qp); quat_exp(&q[3], qq);
    quat_cmul(qp, qq, e);
    quat_log(e, z);
  }
  __device__ static __forceinline__ bool needs_cycles(int solver, const Consts&) { return solver == kSolverNelderMead; }
  struct Prep { double qa[4]; };
  __device__ static __forceinline__ Prep prepare(const Consts& K, const double (&z)[3], const double (&fxc)[6]) {
    Prep P;
    double qF[4], qz[4];
    quat_exp(&fxc[3], qF); quat_exp(z, qz);
    const double sg = K.dir != 0 ? -1.0 : 1.0;
    qz[1] *= sg; qz[2] *= sg; qz[3] *= sg;
    quat_mul(qF, qz, P.qa);
    return P;
  }
  // the residual FUNCTOR at the target rotation qT (unit quaternions: the same rotation R_pᵀ R_q as the 3x3 form of the residual entry points)
  __device__ static __forceinline__ double functor_max(const Consts& K, const double (&z)[3], const double (&qF)[4], const double (&qT)[4]) {
    const bool back = K.dir != 0;
    double X[4], Y[4], g[4], w[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) { X[k] = back ? qT[k] : qF[k]; Y[k] = back ? qF[k] : qT[k]; }
    quat_cmul(X, Y, g); quat_log(g, w);
    return fmax(fabs(z[0] - w[0]), fmax(fabs(z[1] - w[1]), fabs(z[2] - w[2])));
  }
  __device__ static __forceinline__ int verify(const Consts& K, const double (&z)[3], const double (&fxc)[6], const double (&t)[6], const Aux&, double tol) {
    double qF[4], qT[4];
    quat_exp(&fxc[3], qF); quat_exp(&t[3], qT);
    return functor_max(K, z, qF, qT) <= tol ? 0 : 1;
  }
  __device__ static __forceinline__ int gauss_newton(const Consts& K, const Prep& P, const double (&z)[3], const double (&fxc)[6], double (&t)[6],
                                                     int max_iters, double tol) {
    double qF[4], u[4];
    quat_exp(&fxc[3], qF); quat_exp(&t[3], u);
    bool done = false;
    for (int it = 0; it < max_iters; ++it) {
      double e[4];
      quat_cmul(P.qa, u, e);
      // Exp is 1-Lipschitz, so the angle of e is at most |r|₂ <= √3 |r|∞, and 2 |vec e| is at most that angle: a lane with 4 |vec e|² > 3 tol²
      // is not converged whatever the functor's Log is (the rule of P3P3::gauss_newton)
      const double n2e = e[1] * e[1] + e[2] * e[2] + e[3] * e[3];
      const bool undecided = !(4.0 * n2e > 3.0 * tol * tol);
      if (__builtin_amdgcn_ballot_w64(undecided) != 0) done = undecided && functor_max(K, z, qF, u) <= tol;
      if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
      double qn[4];
      quat_mulc(u, e, qn);
      // (renormalised: a product of unit quaternions drifts by an ulp per step; 1/|q| = 3/2 − |q|²/2 to O(eps²))
      const double nn = __builtin_fma(-0.5, qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3], 1.5);
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = done ? u[k] : qn[k] * nn;
    }
    quat_log(u, &t[3]);
    return done ? 0 : 1;
  }
  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts& K, const Prep& P, const double (&z)[3], const double (&fxc)[6],
                                              double (&t)[6], Aux&, int max_iters, double tol) {
    if constexpr (SOLVER == kSolverClosedForm || SOLVER == kSolverNewton) { quat_log(P.qa, &t[3]); return 0; }
    else if constexpr (SOLVER == kSolverGaussNewton) return gauss_newton(K, P, z, fxc, t, max_iters, tol);
    else {
      ROTCost cost;
      cost.z[0] = z[0]; cost.z[1] = z[1]; cost.z[2] = z[2];
      so3_exp(&fxc[3], cost.F); cost.dir = K.dir;
      double x[3] = {t[3], t[4], t[5]};
      const int st = nelder_mead<3>(cost, x, max_iters, tol);
      t[3] = x[0]; t[4] = x[1]; t[5] = x[2];
      return st;
    }
  }
};

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
hipError_t launch_conv_pose3pose3xyyaw(const ConvArgs& a, int solver, hipStream_t s) { return launch_solver<P3XYY>(a, solver, s); }
hipError_t launch_conv_pose3pose3rotation(const ConvArgs& a, int solver, hipStream_t s) { return launch_solver<P3ROT>(a, solver, s); }
hipError_t launch_conv_priorpose3zrp(const ConvArgs& a, hipStream_t s) { return launch_ppl<P3ZRP, kSolverClosedForm>(a, s); }
hipError_t launch_deconv_pose3_partial(int family, const DeconvArgs& a, hipStream_t s) {
  if (family == kDeconvPose3Pose3XYYaw) return launch_deconv_t<P3XYY>(a, s);
  if (family == kDeconvPose3Pose3Rotation) return launch_deconv_t<P3ROT>(a, s);
  return hipErrorInvalidValue;
}

}  // namespace rome
