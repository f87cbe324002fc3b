// rome_blockops.hip -- kernels on whole belief blocks of a store: store <-> device buffer copies (k_scatter_blocks) and the block
// operations ROME_BLOCKOP_* of include/rome_mi355.h on Pose2 / Point2 blocks (k_block_ops) and Pose3 blocks (k_block_ops_pose3).
// Floating-point contraction by source expression, as in the convolution kernels (rome_conv.hpp).
#pragma clang fp contract(on)
#include "../../include/rome_mi355.h"
#include "rome_device_math.hpp"
#include "rome_kernels.h"

namespace rome {

// an entry's first word is type | flags << 8: the inversion flags of a compose entry as bits of `flags`
constexpr int kInvertA = ROME_BLOCKOP_INVERT_A >> 8, kInvertB = ROME_BLOCKOP_INVERT_B >> 8;

// ---- store <-> blocks of a device buffer (the receive side of a frontier exchange / a contiguous download buffer): one 256-thread
//      block per belief
__global__ void __launch_bounds__(256) k_scatter_blocks(int N, const int4* __restrict__ ent, double* buf, long long stride,
                                                        double* d2, double* dpt, double* d3, int to_store) {
  const int4 e = ent[blockIdx.x];   // (dim, var, block, type)
  double* sv = (e.w == 0 ? d2 : (e.w == 1 ? dpt : d3)) + (size_t)e.y * e.x * N;
  double* bb = buf + (size_t)e.z * (size_t)stride;
  if (to_store) { for (int q = threadIdx.x; q < e.x * N; q += 256) sv[q] = bb[q]; }
  else { for (int q = threadIdx.x; q < e.x * N; q += 256) bb[q] = sv[q]; }
}
hipError_t launch_scatter_blocks(int n, int N, const int32_t* ent, const double* buf, int64_t stride, double* st2, double* st_pt, double* st3,
                                 hipStream_t s, int to_store) {
  if (n > 0) hipLaunchKernelGGL(k_scatter_blocks, dim3(n), dim3(256), 0, s, N, reinterpret_cast<const int4*>(ent), const_cast<double*>(buf), (long long)stride,
                                st2, st_pt, st3, to_store);
  return hipGetLastError();
}

// ---- block operations inside a store (copy / anchor / relative / compose): one 256-thread block per entry (type | flags << 8, a, b, dst)
__global__ void __launch_bounds__(256) k_block_ops(int op, int N, const int4* __restrict__ ent, double* d2, double* dpt, double* d3, const double* __restrict__ prm) {
  int4 e = ent[blockIdx.x];
  const int flags = e.x >> 8;   // (compose: kInvertA = take A^-1, kInvertB = take B^-1)
  e.x &= 0xff;
  const int dim = e.x == 0 ? 3 : (e.x == 1 ? 2 : 6);
  double* base = e.x == 0 ? d2 : (e.x == 1 ? dpt : d3);
  const double* A = base + (size_t)e.y * dim * N;
  double* D = base + (size_t)e.w * dim * N;
  const int i = threadIdx.x;
  if (op == ROME_BLOCKOP_COPY) { for (int q = i; q < dim * N; q += 256) D[q] = A[q]; return; }
  if (op == ROME_BLOCKOP_MIX) {   // mix: particle i of D <- particle i of A unless i % k == k - 1 (k = flags): D keeps every k-th particle of its own
    const int k = flags < 1 ? 1 : flags;
    for (int q = i; q < N; q += 256)
      if (q % k != k - 1)
        for (int d = 0; d < dim; ++d) D[(size_t)d * N + q] = A[(size_t)d * N + q];
    return;
  }
  if (op == ROME_BLOCKOP_COMPOSE) {   // compose, particle by particle, Pose2 coordinates (x, y, theta): D_i = A'_i (+) B'_i with A' = A or A^-1, B' = B or B^-1
    const double* Bq = d2 + (size_t)e.z * 3 * N;
    for (int q = i; q < N; q += 256) {
      double ax = A[q], ay = A[N + q], at = A[2 * N + q], bx = Bq[q], by = Bq[N + q], bt = Bq[2 * N + q];
      double sn, cs;
      if (flags & kInvertA) { sincos(at, &sn, &cs); const double x = -(cs * ax + sn * ay), y = -(-sn * ax + cs * ay); ax = x; ay = y; at = -at; }
      if (flags & kInvertB) { sincos(bt, &sn, &cs); const double x = -(cs * bx + sn * by), y = -(-sn * bx + cs * by); bx = x; by = y; bt = -bt; }
      sincos(at, &sn, &cs);
      double s2, c2; sincos(at + bt, &s2, &c2);
      D[q] = ax + cs * bx - sn * by; D[N + q] = ay + sn * bx + cs * by; D[2 * N + q] = atan2(s2, c2);
    }
    const double gt = prm ? prm[2 * (size_t)blockIdx.x] : 1.0, gth = prm ? prm[2 * (size_t)blockIdx.x + 1] : 1.0;
    if (gt == 1.0 && gth == 1.0) return;
    // inflate the deviations of the composed samples about their mean (star-mesh transform: the edge's spread grows by what the pair
    // shares with the other legs of the eliminated star): translation by gt, heading by gth.  Sums in a fixed order (as the anchor).
    __shared__ double rs[4][256];
    __syncthreads();
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int q = i; q < N; q += 256) { double sn, cs; sincos(D[2 * N + q], &sn, &cs); a0 += D[q]; a1 += D[N + q]; a2 += sn; a3 += cs; }
    rs[0][i] = a0; rs[1][i] = a1; rs[2][i] = a2; rs[3][i] = a3;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (i < w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) rs[k][i] += rs[k][i + w];
      }
      __syncthreads();
    }
    const double inv = 1.0 / (double)N, mx = rs[0][0] * inv, my = rs[1][0] * inv, mt = atan2(rs[2][0], rs[3][0]);
    for (int q = i; q < N; q += 256) {
      double sn, cs; sincos(D[2 * N + q] - mt, &sn, &cs);
      const double dt = atan2(sn, cs);
      double s2, c2; sincos(mt + gth * dt, &s2, &c2);
      D[q] = mx + gt * (D[q] - mx); D[N + q] = my + gt * (D[N + q] - my); D[2 * N + q] = atan2(s2, c2);
    }
    return;
  }
  if (op == ROME_BLOCKOP_RELATIVE) {   // relative to ref = particle 0 of the POSE2 block e.y: Pose2 -> tangent coordinates of ref^-1 * s_i; Point2 -> (bearing, range)
    const double* Rf = d2 + (size_t)e.y * 3 * N;
    const double* S = base + (size_t)e.z * dim * N;
    const double rx = Rf[0], ry = Rf[N], rt = Rf[2 * N];
    double sn, cs; sincos(rt, &sn, &cs);
    for (int q = i; q < N; q += 256) {
      const double dx = S[q] - rx, dy = S[N + q] - ry;
      const double lx = cs * dx + sn * dy, ly = -sn * dx + cs * dy;
      if (e.x == 0) {
        double s2, c2; sincos(S[2 * N + q] - rt, &s2, &c2);
        D[q] = lx; D[N + q] = ly; D[2 * N + q] = atan2(s2, c2);
      } else { D[q] = atan2(ly, lx); D[N + q] = sqrt(lx * lx + ly * ly); }
    }
    return;
  }
  // ROME_BLOCKOP_ANCHOR: the mean point, N times.  Sums in a fixed order (lane partials -> LDS tree) so that the result does not depend on scheduling.
  __shared__ double red[8][256];
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = i; q < N; q += 256) {
    if (e.x == 0) { double sn, cs; sincos(A[2 * N + q], &sn, &cs); acc[0] += A[q]; acc[1] += A[N + q]; acc[2] += sn; acc[3] += cs; }
    else if (e.x == 1) { acc[0] += A[q]; acc[1] += A[N + q]; }
    else { acc[0] += A[q]; acc[1] += A[N + q]; acc[2] += A[2 * N + q]; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][i] = acc[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (i < w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][i] += red[k][i + w];
    }
    __syncthreads();
  }
  const double inv = 1.0 / (double)N;
  double m[6];
  if (e.x == 0) { m[0] = red[0][0] * inv; m[1] = red[1][0] * inv; m[2] = atan2(red[2][0], red[3][0]); }
  else if (e.x == 1) { m[0] = red[0][0] * inv; m[1] = red[1][0] * inv; }
  else { m[0] = red[0][0] * inv; m[1] = red[1][0] * inv; m[2] = red[2][0] * inv; m[3] = A[3 * N]; m[4] = A[4 * N]; m[5] = A[5 * N]; }
  __syncthreads();
  for (int q = i; q < dim * N; q += 256) D[q] = m[q / N];
}
hipError_t launch_block_ops(int op, int n, int N, const int32_t* ent, double* st2, double* st_pt, double* st3, hipStream_t s, const double* prm) {
  if (n > 0) hipLaunchKernelGGL(k_block_ops, dim3(n), dim3(256), 0, s, op, N, reinterpret_cast<const int4*>(ent), st2, st_pt, st3, prm);
  return hipGetLastError();
}

// ---- block operations on POSE3 blocks (compose / mean anchor): a kernel of its own with the launch shape of k_block_ops -- one 256-thread
//      block per entry (type | flags << 8, a, b, dst), particles strided by 256.  Store coordinates (t, ω); the rotation is the unit
//      quaternion Exp(ω) from load to store (quat_log: the w >= 0 representative, θ = π snap).
__device__ __forceinline__ void p3_load(const double* P, int N, int q, double (&t)[3], double (&r)[4]) {
  double w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { t[k] = P[(size_t)k * N + q]; w[k] = P[(size_t)(3 + k) * N + q]; }
  quat_exp(w, r);
}
__device__ __forceinline__ void p3_invert(double (&t)[3], double (&r)[4]) {   // (t, q) -> (-R(q)ᵀ t, conj q)
  r[1] = -r[1]; r[2] = -r[2]; r[3] = -r[3];
  double u[3];
  quat_rot(r, t, u);
  t[0] = -u[0]; t[1] = -u[1]; t[2] = -u[2];
}
// the mean point of a Pose3 block: mean translation; rotation q_m = q_0 ⊗ Exp(mean_i Log(conj q_0 ⊗ q_i)) (k_belief_stats, D == 6).
// Sums in a fixed order (lane partials -> LDS tree) so that the result does not depend on scheduling.  Every thread of the block calls it.
__device__ __forceinline__ void p3_block_mean(const double* P, int N, int i, double (*red)[256], double (&tm)[3], double (&qm)[4]) {
  double t0[3], q0[4];
  p3_load(P, N, 0, t0, q0);
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int q = i; q < N; q += 256) {
    double t[3], r[4], e[4], d[3];
    p3_load(P, N, q, t, r);
    quat_cmul(q0, r, e);
    quat_log(e, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) { acc[k] += t[k]; acc[3 + k] += d[k]; }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) red[k][i] = acc[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (i < w) {
#pragma unroll
      for (int k = 0; k < 6; ++k) red[k][i] += red[k][i + w];
    }
    __syncthreads();
  }
  const double inv = 1.0 / (double)N;
  double md[3], qe[4];
#pragma unroll
  for (int k = 0; k < 3; ++k) { tm[k] = red[k][0] * inv; md[k] = red[3 + k][0] * inv; }
  quat_exp(md, qe);
  quat_mul(q0, qe, qm);
}
__global__ void __launch_bounds__(256) k_block_ops_pose3(int op, int N, const int4* __restrict__ ent, double* d3, const double* __restrict__ prm) {
  const int4 e = ent[blockIdx.x];
  const int flags = e.x >> 8;   // (compose: kInvertA = take A^-1, kInvertB = take B^-1)
  const double* A = d3 + (size_t)e.y * 6 * N;
  double* D = d3 + (size_t)e.w * 6 * N;
  const int i = threadIdx.x;
  __shared__ double red[6][256];
  double tm[3], qm[4];
  if (op == ROME_BLOCKOP_ANCHOR_MEAN) {   // mean anchor: N copies of (mean translation, q_m)
    p3_block_mean(A, N, i, red, tm, qm);
    double wm[3];
    quat_log(qm, wm);
    for (int q = i; q < N; q += 256) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { D[(size_t)k * N + q] = tm[k]; D[(size_t)(3 + k) * N + q] = wm[k]; }
    }
    return;
  }
  // compose, particle by particle: D_i = A'_i (+) B'_i = (t_a + R(q_a) t_b, q_a ⊗ q_b) with A' = A or A^-1, B' = B or B^-1
  const double* B = d3 + (size_t)e.z * 6 * N;
  for (int q = i; q < N; q += 256) {
    double ta[3], qa[4], tb[3], qb[4], u[3], qd[4], w[3];
    p3_load(A, N, q, ta, qa);
    p3_load(B, N, q, tb, qb);
    if (flags & kInvertA) p3_invert(ta, qa);
    if (flags & kInvertB) p3_invert(tb, qb);
    quat_rot(qa, tb, u);
    quat_mul(qa, qb, qd);
    quat_log(qd, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) { D[(size_t)k * N + q] = ta[k] + u[k]; D[(size_t)(3 + k) * N + q] = w[k]; }
  }
  const double gt = prm ? prm[2 * (size_t)blockIdx.x] : 1.0, gth = prm ? prm[2 * (size_t)blockIdx.x + 1] : 1.0;
  if (gt == 1.0 && gth == 1.0) return;
  // star-mesh inflation of the deviations of the composed samples about their mean (as k_block_ops does for Pose2): translation by gt,
  // rotation q_i' = q_m ⊗ Exp(gth · Log(conj q_m ⊗ q_i)).  The mean reads the block as stored.
  __syncthreads();
  p3_block_mean(D, N, i, red, tm, qm);
  for (int q = i; q < N; q += 256) {
    double t[3], r[4], dq[4], d[3], qe[4], qn[4], w[3];
    p3_load(D, N, q, t, r);
    quat_cmul(qm, r, dq);
    quat_log(dq, d);
    d[0] *= gth; d[1] *= gth; d[2] *= gth;
    quat_exp(d, qe);
    quat_mul(qm, qe, qn);
    quat_log(qn, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) { D[(size_t)k * N + q] = tm[k] + gt * (t[k] - tm[k]); D[(size_t)(3 + k) * N + q] = w[k]; }
  }
}
hipError_t launch_block_ops_pose3(int op, int n, int N, const int32_t* ent, double* st3, hipStream_t s, const double* prm) {
  if (op != ROME_BLOCKOP_COMPOSE && op != ROME_BLOCKOP_ANCHOR_MEAN) return hipErrorInvalidValue;
  if (n > 0) hipLaunchKernelGGL(k_block_ops_pose3, dim3(n), dim3(256), 0, s, op, N, reinterpret_cast<const int4*>(ent), st3, prm);
  return hipGetLastError();
}

}  // namespace rome
