// rome_rows.hip -- the kernels that work row by row outside a convolution: the prior samplers (one wave per prior), the residual-only
// kernels of the KAT entry points and the native point layout <-> coordinate conversions (one thread per row).
// Floating-point contraction by source expression, as in the convolution kernels (rome_conv.hpp): the residuals round as they do there.
#pragma clang fp contract(on)
#include "rome_device_math.hpp"
#include "rome_kernels.h"

namespace rome {

// ---- prior sampling: out = coords(exp_ϵ(hat(μ + Lξ))) ; one wave per prior
template <int D, int PPL>
__global__ void __launch_bounds__(256) k_sample_prior(const ConvArgs a) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (c >= a.n_conv) return;
  const int N = a.N;
  const int f = a.rows4 ? a.rows4[4 * (size_t)c] : (a.factor ? a.factor[c] : c);   // (clique tables: the factor is column 0 of the row)
  constexpr int NL = D * (D + 1) / 2;
  const double* mu = a.mu + (size_t)D * f;
  const double* L = a.L + (size_t)NL * f;
  double* ob = a.out + (size_t)c * D * N;
  const uint64_t stream = a.stream_offset + (uint64_t)(a.row_stream ? a.row_stream[c] : c);
#pragma unroll(PPL <= 8 ? PPL : 1)
  for (int k = 0; k < PPL; ++k) {
    const int i = lane + 64 * k;
    if (i < N) {
      double xi[D], zc[D];
      if (a.noise) {
#pragma unroll
        for (int d = 0; d < D; ++d) xi[d] = a.noise[(size_t)c * D * N + d * N + i];
      } else rng_normals<D>(a.seed, stream, (uint32_t)i, xi);
      int p = 0;
#pragma unroll
      for (int r = 0; r < D; ++r) {
        double s = mu[r];
#pragma unroll
        for (int j = 0; j <= r; ++j) s += L[p++] * xi[j];
        zc[r] = s;
      }
      if constexpr (D == 3) zc[2] = wrap_pi(zc[2]);
      else if constexpr (D == 6) { Se3 P; se3_from_coords(zc, P); se3_to_coords(P, zc); }   // (D == 2: a Point2, the sample itself)
#pragma unroll
      for (int d = 0; d < D; ++d) ob[d * N + i] = zc[d];
    }
  }
}

// ---- residual-only kernels (rows of AoS coordinates), used by the KAT entry points
__global__ void k_residual_pose2pose2(int n, const double* z, const double* p, const double* q, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Se2 P = se2_from_coords(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
  const Se2 Q = se2_from_coords(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
  double sz, cz; fast_sincos(z[3 * i + 2], &sz, &cz);
  double rr[3];
  residual_pose2pose2(z[3 * i], z[3 * i + 1], cz, sz, P, Q, rr);
  r[3 * i] = rr[0]; r[3 * i + 1] = rr[1]; r[3 * i + 2] = rr[2];
}
__global__ void k_residual_priorpose2(int n, const double* m, const double* p, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Se2 M = se2_from_coords(m[3 * i], m[3 * i + 1], m[3 * i + 2]);
  const Se2 P = se2_from_coords(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
  double rr[3];
  residual_priorpose2(M, P, rr);
  r[3 * i] = rr[0]; r[3 * i + 1] = rr[1]; r[3 * i + 2] = rr[2];
}
// p_is_point: 0 -> p rows are coords (x,y,θ); 1 -> native points [tx,ty,R11,R21,R12,R22]
__global__ void k_residual_bearingrange(int n, const double* z, const double* p, int p_is_point, const double* l, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Se2 P;
  if (p_is_point) { P.x = p[6 * i]; P.y = p[6 * i + 1]; P.c = p[6 * i + 2]; P.s = p[6 * i + 3]; }
  else P = se2_from_coords(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
  double rr[2];
  residual_bearingrange(z[2 * i], z[2 * i + 1], P, l[2 * i], l[2 * i + 1], rr);
  r[2 * i] = rr[0]; r[2 * i + 1] = rr[1];
}
// bearing-only residual; p rows as k_residual_bearingrange
__global__ void k_residual_bearing(int n, const double* z, const double* p, int p_is_point, const double* l, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Se2 P;
  if (p_is_point) { P.x = p[6 * i]; P.y = p[6 * i + 1]; P.c = p[6 * i + 2]; P.s = p[6 * i + 3]; }
  else P = se2_from_coords(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
  r[i] = residual_bearing(z[i], P, l[2 * i], l[2 * i + 1]);
}
// p,q rows are native points (12 doubles: t, R col-major) when pts != 0, else coords (6)
__global__ void k_residual_pose3pose3(int n, const double* z, const double* p, const double* q, int pts, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Se3 P, Q;
  if (pts) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { P.t[k] = p[12 * i + k]; Q.t[k] = q[12 * i + k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) { P.R[k] = p[12 * i + 3 + k]; Q.R[k] = q[12 * i + 3 + k]; }
  } else { se3_from_coords(p + 6 * i, P); se3_from_coords(q + 6 * i, Q); }
  double Z[9], rr[6];
  so3_exp(z + 6 * i + 3, Z);
  residual_pose3pose3(z + 6 * i, Z, P, Q, rr);
#pragma unroll
  for (int k = 0; k < 6; ++k) r[6 * i + k] = rr[k];
}
// Pose3Pose3XYYaw (PartialPose3.jl:116-136): z rows (x, y, θ); p, q rows as k_residual_pose3pose3 (only t_x, t_y and R's first column are read)
__global__ void k_residual_pose3pose3xyyaw(int n, const double* z, const double* p, const double* q, int pts, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Se2 P, Q;
  if (pts) {
    P = se2_of_pose3(p[12 * i], p[12 * i + 1], p[12 * i + 3], p[12 * i + 4]);
    Q = se2_of_pose3(q[12 * i], q[12 * i + 1], q[12 * i + 3], q[12 * i + 4]);
  } else {
    double c[3], u[3];
    so3_col1_dz(p[6 * i + 3], p[6 * i + 4], p[6 * i + 5], c, u); P = se2_of_pose3(p[6 * i], p[6 * i + 1], c[0], c[1]);
    so3_col1_dz(q[6 * i + 3], q[6 * i + 4], q[6 * i + 5], c, u); Q = se2_of_pose3(q[6 * i], q[6 * i + 1], c[0], c[1]);
  }
  double sz, cz; fast_sincos(z[3 * i + 2], &sz, &cz);
  double rr[3];
  residual_pose3pose3xyyaw(z[3 * i], z[3 * i + 1], cz, sz, P, Q, rr);
  r[3 * i] = rr[0]; r[3 * i + 1] = rr[1]; r[3 * i + 2] = rr[2];
}
// Pose3Pose3Rotation (PartialPose3.jl:212-227): z rows are rotation vectors (3); p, q rows as k_residual_pose3pose3 (only the rotations are read)
__global__ void k_residual_pose3pose3rotation(int n, const double* z, const double* p, const double* q, int pts, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double Rp[9], Rq[9];
  if (pts) {
#pragma unroll
    for (int k = 0; k < 9; ++k) { Rp[k] = p[12 * i + 3 + k]; Rq[k] = q[12 * i + 3 + k]; }
  } else { so3_exp(p + 6 * i + 3, Rp); so3_exp(q + 6 * i + 3, Rq); }
  double rr[3];
  residual_pose3pose3rotation(z + 3 * i, Rp, Rq, rr);
  r[3 * i] = rr[0]; r[3 * i + 1] = rr[1]; r[3 * i + 2] = rr[2];
}
__global__ void k_residual_priorpose3(int n, const double* m, const double* p, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Se3 M, P;
  se3_from_coords(m + 6 * i, M); se3_from_coords(p + 6 * i, P);
  double rr[6];
  residual_priorpose3(M, P, rr);
#pragma unroll
  for (int k = 0; k < 6; ++k) r[6 * i + k] = rr[k];
}

// range residuals r = ρ − ‖lm − x‖: x rows are Point2 (dx = 2) or Pose2 coordinates (dx = 3, the heading is not read)
__global__ void k_residual_range(int n, const double* z, const double* x, int dx, const double* l, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  r[i] = z[i] - range_norm(l[2 * i] - x[(size_t)dx * i], l[2 * i + 1] - x[(size_t)dx * i + 1]);
}

// ---- native point layouts <-> coordinates (rows): Pose2 [tx,ty,R11,R21,R12,R22] <-> (x,y,θ);
//      Pose3 [t(3), R col-major(9)] <-> (t, ω).  vee(log(ϵ,p)) / exp_ϵ(hat c) of src/variables/VariableTypes.jl:35,47.
__global__ void k_points_to_coords(int n, int dim, const double* __restrict__ pts, double* __restrict__ c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (dim == 3) {
    c[3 * i] = pts[6 * i]; c[3 * i + 1] = pts[6 * i + 1]; c[3 * i + 2] = atan2(pts[6 * i + 3], pts[6 * i + 2]);
  } else {
    c[6 * i] = pts[12 * i]; c[6 * i + 1] = pts[12 * i + 1]; c[6 * i + 2] = pts[12 * i + 2];
    double R[9], w[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = pts[12 * i + 3 + k];
    so3_log(R, w);
    c[6 * i + 3] = w[0]; c[6 * i + 4] = w[1]; c[6 * i + 5] = w[2];
  }
}
__global__ void k_coords_to_points(int n, int dim, const double* __restrict__ c, double* __restrict__ pts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (dim == 3) {
    double s, co; fast_sincos(c[3 * i + 2], &s, &co);
    pts[6 * i] = c[3 * i]; pts[6 * i + 1] = c[3 * i + 1];
    pts[6 * i + 2] = co; pts[6 * i + 3] = s; pts[6 * i + 4] = -s; pts[6 * i + 5] = co;
  } else {
    pts[12 * i] = c[6 * i]; pts[12 * i + 1] = c[6 * i + 1]; pts[12 * i + 2] = c[6 * i + 2];
    double R[9];
    so3_exp(c + 6 * i + 3, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) pts[12 * i + 3 + k] = R[k];
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <int D>
static hipError_t launch_prior(const ConvArgs& a, hipStream_t s) {
  const int nb = (a.n_conv + 3) / 4;
  if (nb == 0) return hipSuccess;
  if (a.N <= 64)       hipLaunchKernelGGL((k_sample_prior<D, 1>), dim3(nb), dim3(256), 0, s, a);
  else if (a.N <= 128) hipLaunchKernelGGL((k_sample_prior<D, 2>), dim3(nb), dim3(256), 0, s, a);
  else if (a.N <= 256) hipLaunchKernelGGL((k_sample_prior<D, 4>), dim3(nb), dim3(256), 0, s, a);
  else if (a.N <= 512) hipLaunchKernelGGL((k_sample_prior<D, 8>), dim3(nb), dim3(256), 0, s, a);
  else if (a.N <= 4096) hipLaunchKernelGGL((k_sample_prior<D, 64>), dim3(nb), dim3(256), 0, s, a);   // (a runtime-bounded loop over 64 slots)
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t launch_sample_priorpose2(const ConvArgs& a, hipStream_t s) { return launch_prior<3>(a, s); }
hipError_t launch_sample_priorpose3(const ConvArgs& a, hipStream_t s) { return launch_prior<6>(a, s); }
hipError_t launch_sample_priorpoint2(const ConvArgs& a, hipStream_t s) { return launch_prior<2>(a, s); }

// one thread per row, 256 per block: the shape of every launcher below (n == 0 launches nothing)
template <class... P, class... A>
static hipError_t launch_rows(void (*k)(int, P...), int n, hipStream_t s, A... args) {
  if (n > 0) hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, s, n, args...);
  return hipGetLastError();
}
hipError_t launch_residual_pose2pose2(int n, const double* z, const double* p, const double* q, double* r, hipStream_t s) {
  return launch_rows(k_residual_pose2pose2, n, s, z, p, q, r);
}
hipError_t launch_residual_priorpose2(int n, const double* m, const double* p, double* r, hipStream_t s) {
  return launch_rows(k_residual_priorpose2, n, s, m, p, r);
}
hipError_t launch_residual_bearingrange(int n, const double* z, const double* p, int p_is_point, const double* l, double* r, hipStream_t s) {
  return launch_rows(k_residual_bearingrange, n, s, z, p, p_is_point, l, r);
}
hipError_t launch_residual_pose3pose3(int n, const double* z, const double* p, const double* q, int pts, double* r, hipStream_t s) {
  return launch_rows(k_residual_pose3pose3, n, s, z, p, q, pts, r);
}
hipError_t launch_residual_pose3pose3xyyaw(int n, const double* z, const double* p, const double* q, int pts, double* r, hipStream_t s) {
  return launch_rows(k_residual_pose3pose3xyyaw, n, s, z, p, q, pts, r);
}
hipError_t launch_residual_pose3pose3rotation(int n, const double* z, const double* p, const double* q, int pts, double* r, hipStream_t s) {
  return launch_rows(k_residual_pose3pose3rotation, n, s, z, p, q, pts, r);
}
hipError_t launch_residual_priorpose3(int n, const double* m, const double* p, double* r, hipStream_t s) {
  return launch_rows(k_residual_priorpose3, n, s, m, p, r);
}
hipError_t launch_residual_range(int n, const double* z, const double* x, int dx, const double* l, double* r, hipStream_t s) {
  return launch_rows(k_residual_range, n, s, z, x, dx, l, r);
}
hipError_t launch_residual_bearing(int n, const double* z, const double* p, int p_is_point, const double* l, double* r, hipStream_t s) {
  return launch_rows(k_residual_bearing, n, s, z, p, p_is_point, l, r);
}
hipError_t launch_points_to_coords(int n, int dim, const double* pts, double* c, hipStream_t s) {
  return launch_rows(k_points_to_coords, n, s, dim, pts, c);
}
hipError_t launch_coords_to_points(int n, int dim, const double* c, double* pts, hipStream_t s) {
  return launch_rows(k_coords_to_points, n, s, dim, c, pts);
}

}  // namespace rome
