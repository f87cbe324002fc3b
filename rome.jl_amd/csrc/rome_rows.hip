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

// ---- residual-only kernel (rows of AoS coordinates), used by the KAT entry points: thread i reads row i of the measurements z and of
// the variables a, b (b absent: a prior), evaluates R on them and writes row i of r.  Each R states its row widths and evaluates one row.
template <class R>
__global__ void k_residual(int n, const double* z, const double* a, const double* b, double* r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double rr[R::RW];
  R::eval(z + (size_t)R::ZW * i, a + (size_t)R::AW * i, b + (size_t)R::BW * i, rr);
#pragma unroll
  for (int k = 0; k < R::RW; ++k) r[(size_t)R::RW * i + k] = rr[k];
}

// a pose row: coordinates (Pose2 (x, y, θ); Pose3 (t, ω)), or with PTS the native point (Pose2 [tx,ty,R11,R21,R12,R22]; Pose3 [t, R col-major])
template <bool PTS>
__device__ inline Se2 pose2_row(const double* p) {
  if constexpr (PTS) { Se2 P; P.x = p[0]; P.y = p[1]; P.c = p[2]; P.s = p[3]; return P; }
  else return se2_from_coords(p[0], p[1], p[2]);
}
template <bool PTS>
__device__ inline void pose3_row(const double* p, Se3& P) {
  if constexpr (PTS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) P.t[k] = p[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) P.R[k] = p[3 + k];
  } else se3_from_coords(p, P);
}

struct ResPose2Pose2 {
  static constexpr int ZW = 3, AW = 3, BW = 3, RW = 3;
  static __device__ void eval(const double* z, const double* p, const double* q, double (&r)[RW]) {
    const Se2 P = pose2_row<false>(p), Q = pose2_row<false>(q);
    double sz, cz; fast_sincos(z[2], &sz, &cz);
    residual_pose2pose2(z[0], z[1], cz, sz, P, Q, r);
  }
};
struct ResPriorPose2 {
  static constexpr int ZW = 3, AW = 3, BW = 0, RW = 3;
  static __device__ void eval(const double* m, const double* p, const double*, double (&r)[RW]) {
    residual_priorpose2(pose2_row<false>(m), pose2_row<false>(p), r);
  }
};
template <bool PTS>
struct ResBearingRange {
  static constexpr int ZW = 2, AW = PTS ? 6 : 3, BW = 2, RW = 2;
  static __device__ void eval(const double* z, const double* p, const double* l, double (&r)[RW]) {
    residual_bearingrange(z[0], z[1], pose2_row<PTS>(p), l[0], l[1], r);
  }
};
template <bool PTS>
struct ResBearing {
  static constexpr int ZW = 1, AW = PTS ? 6 : 3, BW = 2, RW = 1;
  static __device__ void eval(const double* z, const double* p, const double* l, double (&r)[RW]) {
    r[0] = residual_bearing(z[0], pose2_row<PTS>(p), l[0], l[1]);
  }
};
template <bool PTS>
struct ResPose3Pose3 {
  static constexpr int ZW = 6, AW = PTS ? 12 : 6, BW = AW, RW = 6;
  static __device__ void eval(const double* z, const double* p, const double* q, double (&r)[RW]) {
    Se3 P, Q;
    pose3_row<PTS>(p, P); pose3_row<PTS>(q, Q);
    double Z[9];
    so3_exp(z + 3, Z);
    residual_pose3pose3(z, Z, P, Q, r);
  }
};
// Pose3Pose3XYYaw (PartialPose3.jl:116-136): z rows (x, y, θ); of p and q only t_x, t_y and R's first column are read
template <bool PTS>
struct ResPose3Pose3XYYaw {
  static constexpr int ZW = 3, AW = PTS ? 12 : 6, BW = AW, RW = 3;
  static __device__ Se2 project(const double* p) {
    if constexpr (PTS) return se2_of_pose3(p[0], p[1], p[3], p[4]);
    else { double c[3], u[3]; so3_col1_dz(p[3], p[4], p[5], c, u); return se2_of_pose3(p[0], p[1], c[0], c[1]); }
  }
  static __device__ void eval(const double* z, const double* p, const double* q, double (&r)[RW]) {
    const Se2 P = project(p), Q = project(q);
    double sz, cz; fast_sincos(z[2], &sz, &cz);
    residual_pose3pose3xyyaw(z[0], z[1], cz, sz, P, Q, r);
  }
};
// Pose3Pose3Rotation (PartialPose3.jl:212-227): z rows are rotation vectors; of p and q only the rotations are read
template <bool PTS>
struct ResPose3Pose3Rotation {
  static constexpr int ZW = 3, AW = PTS ? 12 : 6, BW = AW, RW = 3;
  static __device__ void rotation(const double* p, double* R) {
    if constexpr (PTS) {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = p[3 + k];
    } else so3_exp(p + 3, R);
  }
  static __device__ void eval(const double* z, const double* p, const double* q, double (&r)[RW]) {
    double Rp[9], Rq[9];
    rotation(p, Rp); rotation(q, Rq);
    residual_pose3pose3rotation(z, Rp, Rq, r);
  }
};
struct ResPriorPose3 {
  static constexpr int ZW = 6, AW = 6, BW = 0, RW = 6;
  static __device__ void eval(const double* m, const double* p, const double*, double (&r)[RW]) {
    Se3 M, P;
    pose3_row<false>(m, M); pose3_row<false>(p, P);
    residual_priorpose3(M, P, r);
  }
};
// range residuals r = ρ − ‖lm − x‖: x rows are Point2 (DX = 2) or Pose2 coordinates (DX = 3, the heading is not read)
template <int DX>
struct ResRange {
  static constexpr int ZW = 1, AW = DX, BW = 2, RW = 1;
  static __device__ void eval(const double* z, const double* x, const double* l, double (&r)[RW]) {
    r[0] = z[0] - range_norm(l[0] - x[0], l[1] - x[1]);
  }
};

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
// kind: kRes* (rome_kernels.h); pts: the pose rows are native points (the kinds that read a pose's rotation or heading)
hipError_t launch_residual(int kind, int pts, int n, const double* z, const double* a, const double* b, double* r, hipStream_t s) {
  auto go = [&](auto R) { return launch_rows(k_residual<decltype(R)>, n, s, z, a, b, r); };
  switch (kind) {
    case kResPose2Pose2: if (!pts) return go(ResPose2Pose2{}); break;
    case kResPriorPose2: if (!pts) return go(ResPriorPose2{}); break;
    case kResBearingRange: return pts ? go(ResBearingRange<true>{}) : go(ResBearingRange<false>{});
    case kResBearing: return pts ? go(ResBearing<true>{}) : go(ResBearing<false>{});
    case kResPose3Pose3: return pts ? go(ResPose3Pose3<true>{}) : go(ResPose3Pose3<false>{});
    case kResPose3Pose3XYYaw: return pts ? go(ResPose3Pose3XYYaw<true>{}) : go(ResPose3Pose3XYYaw<false>{});
    case kResPose3Pose3Rotation: return pts ? go(ResPose3Pose3Rotation<true>{}) : go(ResPose3Pose3Rotation<false>{});
    case kResPriorPose3: if (!pts) return go(ResPriorPose3{}); break;
    case kResPoint2Point2Range: if (!pts) return go(ResRange<2>{}); break;
    case kResPose2Point2Range: if (!pts) return go(ResRange<3>{}); break;
  }
  return hipErrorInvalidValue;
}
hipError_t launch_points_to_coords(int n, int dim, const double* pts, double* c, hipStream_t s) {
  return launch_rows(k_points_to_coords, n, s, dim, pts, c);
}
hipError_t launch_coords_to_points(int n, int dim, const double* c, double* pts, hipStream_t s) {
  return launch_rows(k_coords_to_points, n, s, dim, c, pts);
}

}  // namespace rome
