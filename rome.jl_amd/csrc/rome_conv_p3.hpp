// rome_conv_p3.hpp -- the Pose3Pose3 (+ PriorPose3 rows) policy.  rome_conv_pose3.hip instantiates the convolution kernels on it; the partial
// Pose3 policies of rome_conv_pose3_partial.hip take its start-point state and its spread (the statistic over all six coordinates).
#pragma once
#include "rome_conv.hpp"

namespace rome {

// ---- Pose3Pose3.  Belief blocks hold coordinates (t, ω); inside the kernel the rotation of every particle lives as a
// unit quaternion (Aux) from load to store, so the inflation cycles never go through Exp/Log round trips, and the root
// (a, qa) of the residual  r = ( p.t + R_p z_t − q.t , Log(R_qᵀ R_p Exp(z_ω)) )  is prepared once per particle:
//   dir 0 (solve q): qa = q_p ⊗ q_z,        a = p.t + R_p z_t   (the root itself)
//   dir 1 (solve p): qa = q_q ⊗ conj(q_z),  a = q.t             (root translation = a − R(qa) z_t)
// The Newton rotation residual is conj(q_T) ⊗ qa: the same angle as the reference's Log(R_qᵀ R_p Z) (for dir 1 the
// vector is that residual rotated by Z, which changes neither its norm nor the root).
// Nelder-Mead mode evaluates Σr² through 3x3 frames, the residual exactly as src/factors/Pose3Pose3.jl:17-29 composes it
// (measured: 191 ms per helix sweep against 264 ms for a quaternion cost, whose inverse-trig call raises the register
// pressure of the 32 inlined evaluations; the Newton / closed-form modes never evaluate a Log).
struct P3P3Cost {
  double zt[3]; double Z[9]; Se3 F; int dir;
  __device__ __forceinline__ double operator()(const double (&x)[6]) const {
    Se3 T; se3_from_coords(x, T);
    double r[6];
    if (dir == 0) residual_pose3pose3(zt, Z, F, T, r); else residual_pose3pose3(zt, Z, T, F, r);
    double s = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += r[k] * r[k];
    return s;
  }
};

struct P3P3 {
  static constexpr int DF = 6, DT = 6, DZ = 6, NL = 21, NK = 27;
  static constexpr int kHypoDir = -1;
  static constexpr bool kUniqueRoot = true;
  struct Consts { double mu[6]; const double* L; int dir; };
  __device__ static __forceinline__ Consts load(const ConvArgs& a, int f, int dr) {
    Consts K;
#pragma unroll
    for (int k = 0; k < 6; ++k) K.mu[k] = a.mu[6 * f + k];
    K.L = a.L + 21 * (size_t)f;  // 21 wave-uniform doubles, read through the scalar cache at use
    K.dir = dr;
    return K;
  }
  __device__ static __forceinline__ Consts from_lds(const double* sk, int dr) {
    Consts K;
#pragma unroll
    for (int k = 0; k < 6; ++k) K.mu[k] = sk[k];
    K.L = sk + 6;
    K.dir = dr;
    return K;
  }
  __device__ static __forceinline__ void measurement(const Consts& K, const double (&xi)[6], double (&z)[6]) {
    int p = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = K.mu[k];
#pragma unroll
      for (int j = 0; j <= k; ++j) s += K.L[p++] * xi[j];
      z[k] = s;
    }
  }
  // the measurement at which the residual vanishes on the pair (k_deconv): z_t = R_pᵀ (q.t − p.t), z_ω = Log(R_pᵀ R_q), the principal
  // rotation vector; R_p is formed once, as a unit quaternion, and serves both parts
  __device__ static __forceinline__ void predict(const double (&p)[6], const double (&q)[6], double (&z)[6]) {
    double qp[4], qq[4], e[4], v[3];
    quat_exp(&p[3], qp); quat_exp(&q[3], qq);
    const double cp[4] = {qp[0], -qp[1], -qp[2], -qp[3]};
    const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    quat_rot(cp, d, v);
    z[0] = v[0]; z[1] = v[1]; z[2] = v[2];
    quat_cmul(qp, qq, e);
    quat_log(e, &z[3]);
  }
  __device__ static __forceinline__ void canonical(double (&)[6]) {}   // finalize() writes the principal rotation vector
  __device__ static __forceinline__ bool needs_cycles(int solver, const Consts& K) {
    return solver == kSolverNelderMead && K.dir != kDirPrior;
  }
  struct Aux { double q[4]; };
  // start point u0 -> state.  The reference takes X0c = vee(log(ϵ, u0)) of the start point, and Manifolds' log returns θ = π exactly
  // for rotations with cos θ + 1 <= √eps: the same snap is applied to the quaternion (w = 0, unit vector part).
  __device__ static __forceinline__ Aux init_aux(const double (&t)[6]) {
    Aux A; quat_exp(&t[3], A.q);
    if (2.0 * A.q[0] * A.q[0] <= kSqrtEps) {
      const double inv = 1.0 / fast_sqrt(A.q[1] * A.q[1] + A.q[2] * A.q[2] + A.q[3] * A.q[3]);
      A.q[0] = 0.0; A.q[1] *= inv; A.q[2] *= inv; A.q[3] *= inv;
    }
    return A;
  }
  __device__ static __forceinline__ void finalize(double (&t)[6], const Aux& A) { quat_log(A.q, &t[3]); }
  struct Ref { double c[3]; double q[4]; };
  __device__ static __forceinline__ Ref make_ref(const double (&t0)[6], const Aux& A0) {
    return Ref{{t0[0], t0[1], t0[2]}, {A0.q[0], A0.q[1], A0.q[2], A0.q[3]}};
  }
  __device__ static __forceinline__ void tangent(const Ref& r, const double (&t)[6], const Aux& A, double (&d)[6]) {
    double e[4];
    quat_cmul(r.q, A.q, e); quat_log(e, d + 3);
    d[0] = t[0] - r.c[0]; d[1] = t[1] - r.c[1]; d[2] = t[2] - r.c[2];
  }

  // std of the tangent coordinates about particle 0: translation differences and Log(R0ᵀ R_i)
  template <int PPL>
  __device__ static __forceinline__ double spread(const double (&t)[PPL][6], const Aux (&A)[PPL], const bool (&act)[PPL], double inv, double den) {
    double c0[3], q0[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) c0[k] = readlane_f64(t[0][k], 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) q0[k] = readlane_f64(A[0].q[k], 0);
    double s[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) s[j] = 0.0;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      double e[4], d[6];
      quat_cmul(q0, A[k].q, e); quat_log(e, d + 3);
      d[0] = t[k][0] - c0[0]; d[1] = t[k][1] - c0[1]; d[2] = t[k][2] - c0[2];
      if (act[k]) {
#pragma unroll
        for (int j = 0; j < 6; ++j) { s[2 * j] += d[j]; s[2 * j + 1] += d[j] * d[j]; }
      }
    }
    wave_sum_n<12>(s);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) acc += fmax(0.0, (s[2 * j + 1] - s[2 * j] * s[2 * j] * inv) * den);
    return fast_sqrt(acc);
  }
  // The root (a, qa) of the residual, prepared once per particle for both directions (cf. P2P2::Prep): with the rotation
  // solved first, the translation residual is affine with R at the root rotation, so R(qa) z_t is loop-invariant:
  //   dir 0 (solve q): qa = q_p ⊗ q_z,        a = p.t + R_p z_t
  //   dir 1 (solve p): qa = q_q ⊗ conj(q_z),  a = q.t − R(qa) z_t
  //   prior row:       qa = Exp(z_ω),          a = z_t
  struct Prep { double a[3], qa[4]; };
  __device__ static __forceinline__ Prep prepare(const Consts& K, const double (&z)[6], const double (&fxc)[6]) {
    Prep P;
    double qz[4];
    quat_exp(&z[3], qz);
    if (K.dir == kDirPrior) {  // PriorPose3 row: the sample point exp_ϵ(hat z)
#pragma unroll
      for (int k = 0; k < 3; ++k) P.a[k] = z[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) P.qa[k] = qz[k];
      return P;
    }
    // both directions in ONE branch-free form (a wave of the packed sweep spans rows of both; cf. P2P2::prepare):
    //   qa = q_F (x) (dir 1 ? conj(q_z) : q_z),   a = F.t +- R(dir 1 ? qa : q_F) z_t
    double qF[4], v[3], qs[4], qr[4];
    quat_exp(&fxc[3], qF);
    const bool back = K.dir != 0;
    const double sg = back ? -1.0 : 1.0;
    qs[0] = qz[0]; qs[1] = sg * qz[1]; qs[2] = sg * qz[2]; qs[3] = sg * qz[3];
    quat_mul(qF, qs, P.qa);
#pragma unroll
    for (int k = 0; k < 4; ++k) qr[k] = back ? P.qa[k] : qF[k];
    quat_rot(qr, z, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) P.a[k] = __builtin_fma(sg, v[k], fxc[k]);
    return P;
  }
  // u0 ∘ exp_ϵ(hat e), e = spread·(u − ½):  t += R e_t,  R ← R Exp(e_ω)
  __device__ static __forceinline__ void add_entropy(double (&t)[6], Aux& A, double spread, const double (&u)[6]) {
    double e[6], v[3], qe[4], qn[4];
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = spread * (u[k] - 0.5);
    quat_rot(A.q, e, v);
    t[0] += v[0]; t[1] += v[1]; t[2] += v[2];
    quat_exp(e + 3, qe); quat_mul(A.q, qe, qn);
#pragma unroll
    for (int k = 0; k < 4; ++k) A.q[k] = qn[k];
  }
  // the residual FUNCTOR itself (src/factors/Pose3Pose3.jl:17-29 / Pose3D.jl:15-19, through 3x3 frames) at the target (t, R(q))
  __device__ static __forceinline__ void quat_to_mat(const double (&q)[4], double* R) {   // column-major
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y + w * z);       R[2] = 2.0 * (x * z - w * y);
    R[3] = 2.0 * (x * y - w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z + w * x);
    R[6] = 2.0 * (x * z + w * y);       R[7] = 2.0 * (y * z - w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
  }
  __device__ static __forceinline__ void functor(const Consts& K, const double (&z)[6], const double* Z, const Se3& F, const Se3& T, double (&r)[6]) {
    if (K.dir == kDirPrior) { Se3 M; se3_from_coords(z, M); residual_priorpose3(M, T, r); }
    else if (K.dir == 0) residual_pose3pose3(z, Z, F, T, r);
    else residual_pose3pose3(z, Z, T, F, r);
  }
  __device__ static __forceinline__ int verify(const Consts& K, const double (&z)[6], const double (&fxc)[6], const double (&t)[6], const Aux& A, double tol) {
    // ONE branch-free evaluation for the three row kinds, on unit quaternions (the predicted-pose residual of gauss_newton below: the
    // functor's residual up to the sign of both parts; round 6 -- the 3x3 functor evaluated under three divergent branches cost 44 us of
    // the 92 us of a helix sweep with a status array): S = the pose the factor predicts for q (dir 1: from the returned p), G = q
    const bool back = K.dir == 1, prior = K.dir == kDirPrior;
    double qz[4], qF[4], Ft[3];
    quat_exp(&z[3], qz);
    quat_exp(&fxc[3], qF);
#pragma unroll
    for (int k = 0; k < 4; ++k) qF[k] = prior ? (k == 0 ? 1.0 : 0.0) : qF[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Ft[k] = prior ? 0.0 : fxc[k];
    double X[4], M[4], v[3], G[4], e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { X[k] = back ? A.q[k] : qF[k]; G[k] = back ? qF[k] : A.q[k]; }
    quat_mul(X, qz, M); quat_rot(X, z, v);
    quat_cmul(M, G, e);
    double mt = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) mt = fmax(mt, fabs((back ? Ft[k] : t[k]) - ((back ? t[k] : Ft[k]) + v[k])));
    const double n2e = e[1] * e[1] + e[2] * e[2] + e[3] * e[3];
    if (mt > tol || 4.0 * n2e > 3.0 * tol * tol) return 1;    // |r_w|_inf >= 2 |vec e| / sqrt 3: not converged whatever the Log is
    double rw[3];
    if (n2e > 1e-16) quat_log(e, rw);                           // (only with a tolerance above 1e-8)
    else { const double k2 = 2.0 * fast_rcp(e[0]); rw[0] = k2 * e[1]; rw[1] = k2 * e[2]; rw[2] = k2 * e[3]; }
    return fmax(mt, fmax(fabs(rw[0]), fmax(fabs(rw[1]), fabs(rw[2])))) <= tol ? 0 : 1;
  }
  // Gauss-Newton on the functor (the oracle's p3p3_newton_pt): right-perturbation updates on the group that zero the residual,
  //   dir 0: R_q <- R_q Exp(r_w), q.t += r_t;   dir 1: R_p <- R_p Exp(-Z r_w), p.t <- q.t - R_p z_t
  // Round 6: the residual is evaluated ON UNIT QUATERNIONS -- r_w = Log(conj(q_q) (x) q_p (x) q_z), the same rotation as the functor's
  // Log(R_q^T R_p Exp(z_w)) (src/factors/Pose3Pose3.jl:17-29; the 3x3 form stays in `functor` / `verify` and the residual entry points),
  // r_t = p.t + R(q_p) z_t - q.t -- and the update is applied with the residual ROTATION e itself instead of Exp(Log(e)):
  //   dir 0: q_q <- q_q (x) e;   dir 1: Exp(-Z r_w) = q_z (x) conj(e) (x) conj(q_z), so q_p <- (q_p (x) q_z) (x) conj(e) (x) conj(q_z)
  // (the P2P2 iteration carries (cos, sin) the same way).  What an iterate costs: two or three quaternion products and one Log -- whose
  // inverse-trigonometric branch is skipped when every lane of the wave is at |vec e| < 1e-8 (Log e = 2 vec e / e_w to 1e-24: the
  // verification iterate) -- instead of a 3x3 frame from the quaternion, two 3x3 products, the matrix Log and an Exp per iterate
  // (the packed sweep on the 10k helix: 154.5 -> 102 us with this alone; profiles/r06_p3p3_gn.md).
  __device__ static __forceinline__ void quat_log_iter(const double (&q)[4], double* w) {
    const double n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (__builtin_amdgcn_ballot_w64(n2 > 1e-16) == 0) {   // wave-uniform: every active lane is at the root already
      const double k = 2.0 * fast_rcp(q[0]);
      w[0] = k * q[1]; w[1] = k * q[2]; w[2] = k * q[3];
      return;
    }
    quat_log(q, w);
  }
  // ONE loop body for both directions (a wave of the packed sweep spans rows of both: two branches would run one after the other).  The
  // iteration lives in the PREDICTED pose of q: (s, u) with target (Ts, Tu),
  //   dir 0 / prior:  (s, u) = (q.t, q_q) itself,                         target = F o exp(z) = (F.t + R_F z_t, q_F (x) q_z)
  //   dir 1:          (s, u) = (p.t + R_p z_t, q_p (x) q_z) of the iterate p,  target = the fixed q = (F.t, q_F)
  // residual e = conj(u) (x) Tu, r_t = Ts - s (dir 1: the functor's residual up to the sign of both parts -- the test is on max|r|);
  // update u <- u (x) e, s <- s + r_t.  In dir 1 this IS R_p <- R_p Exp(-Z r_w), p.t <- q.t - R_p z_t: u (x) e (x) conj(q_z) = q_p (x) q_z
  // (x) conj(e') (x) conj(q_z) with e' the functor's rotation.  The iterate p is recovered from (s, u) once, after the loop.
  __device__ static __forceinline__ int gauss_newton(const Consts& K, const double (&z)[6], const double (&fxc)[6], double (&t)[6], Aux& A, int max_iters, double tol) {
    const bool back = K.dir == 1, prior = K.dir == kDirPrior;
    double qz[4], qF[4], Ft[3];
    quat_exp(&z[3], qz);
    quat_exp(&fxc[3], qF);
#pragma unroll
    for (int k = 0; k < 4; ++k) qF[k] = prior ? (k == 0 ? 1.0 : 0.0) : qF[k];   // (prior row: the identity pose)
#pragma unroll
    for (int k = 0; k < 3; ++k) Ft[k] = prior ? 0.0 : fxc[k];
    // M = X (x) q_z, v = R(X) z_t with X = the fixed rotation (dir 0: the target's) or the start iterate's (dir 1: the state's)
    double X[4], M[4], v[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) X[k] = back ? A.q[k] : qF[k];
    quat_mul(X, qz, M); quat_rot(X, z, v);
    double u[4], Tu[4], s[3], Ts[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) { u[k] = back ? M[k] : A.q[k]; Tu[k] = back ? qF[k] : M[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[k] = back ? t[k] + v[k] : t[k]; Ts[k] = back ? Ft[k] : Ft[k] + v[k]; }
    int st = 1;
    for (int it = 0; it < max_iters; ++it) {
      double e[4], r[6];
      quat_cmul(u, Tu, e);
      r[0] = Ts[0] - s[0]; r[1] = Ts[1] - s[1]; r[2] = Ts[2] - s[2];
      // The coordinates Log(e) are needed only where the test max|r| <= tol can pass: |r_w|_inf >= theta / sqrt 3 >= 2 |vec e| / sqrt 3, so
      // a lane with 4 |vec e|^2 > 3 tol^2 (or a translation residual above tol) is NOT converged whatever its Log is -- the same
      // decision without the inverse-trigonometric evaluation.  Wave-uniform: the start iterate skips the Log, the verification
      // iterate takes its small-angle branch (quat_log_iter); the full Log runs only for a wave with a lane in between.
      const double mt = fmax(fabs(r[0]), fmax(fabs(r[1]), fabs(r[2])));
      const double n2e = e[1] * e[1] + e[2] * e[2] + e[3] * e[3];
      const bool undecided = !(mt > tol) && !(4.0 * n2e > 3.0 * tol * tol);
      if (__builtin_amdgcn_ballot_w64(undecided) != 0) {
        quat_log_iter(e, r + 3);
        if (fmax(mt, fmax(fabs(r[3]), fmax(fabs(r[4]), fabs(r[5])))) <= tol) { st = 0; break; }
      }
      double qn[4];
      quat_mul(u, e, qn);
      s[0] += r[0]; s[1] += r[1]; s[2] += r[2];
      // (renormalised: a product of unit quaternions drifts by an ulp per step; |q|^2 = 1 + eps, 1/|q| = 3/2 - |q|^2/2 to O(eps^2))
      const double nn = __builtin_fma(-0.5, qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3], 1.5);
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = qn[k] * nn;
    }
    // the iterate itself: dir 0 / prior (s, u); dir 1  q_p = u (x) conj(q_z), p.t = s - R(q_p) z_t
    double qp[4], w[3];
    quat_mulc(u, qz, qp); quat_rot(qp, z, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) A.q[k] = back ? qp[k] : u[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = back ? s[k] - w[k] : s[k];
    return st;
  }
  template <int SOLVER>
  __device__ static __forceinline__ int solve(const Consts& K, const Prep& P, const double (&z)[6], const double (&fxc)[6],
                                              double (&t)[6], Aux& A, int max_iters, double tol) {
    int st = 0;
    if (K.dir == kDirPrior || SOLVER == kSolverClosedForm || SOLVER == kSolverNewton) {   // the prepared root itself
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = P.a[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) A.q[k] = P.qa[k];
      return 0;
    }
    if constexpr (SOLVER == kSolverGaussNewton) st = gauss_newton(K, z, fxc, t, A, max_iters, tol);
    else if constexpr (SOLVER == kSolverNelderMead) {
      P3P3Cost cost;
#pragma unroll
      for (int k = 0; k < 3; ++k) cost.zt[k] = z[k];
      so3_exp(&z[3], cost.Z);
      se3_from_coords(fxc, cost.F);
      cost.dir = K.dir;
      quat_log(A.q, &t[3]);   // X0c = vee(log(ϵ,u0)): Nelder-Mead works on the (t, ω) coordinates
      st = nelder_mead<6>(cost, t, max_iters, tol);
      quat_exp(&t[3], A.q);
    }
    return st;
  }
};

}  // namespace rome
