// rome_product_partial.hip -- stage 2 of the partial-aware product: per-coordinate 1-D products.
//
// A partial factor (Pose3Pose3XYYaw, PriorPose3ZRP, Pose2Point2Range towards the pose) solves some coordinates of its target and passes
// the others through.  Stage 1 -- the existing product over the FULL proposal rows only -- has left its result J in `bel`.  Here every
// coordinate c of a variable v that at least one partial row covers is one task: the 1-D importance product (the D = 1 case of the
// definition above ro_product_bw in oracle/rome_oracle.c) of the marginals prop[r][c][0..N) of the partial rows covering c, in CSR
// order, and -- when v has full rows -- of the marginal J[v][c][.] last.  One density: a bit copy.  Coordinates nobody covers keep J.
//
//  * k_product_coord<S>: one wave (64-thread block) per task; lane l owns base points l, l + 64, ... (S slots, N <= 64·S); kernel points
//    are walked at a wave-uniform address (scalar-cache loads of `prop`, LDS broadcasts of J).  The line bel[v][c][.] belongs to this
//    wave alone: it is staged in LDS before anything is stored, so `bel` is updated in place with wave-level ordering only -- no
//    inter-block communication, no atomics.  Weights are scanned in point order and looked up by bisection, as k_product does, so the
//    picks are those of a sequential CPU scan.
#include "rome_device_math.hpp"
#include "rome_kernels.h"

#include <cmath>

namespace rome {

constexpr int kCoordMaxN = 512;

struct CoordArgs {
  int T, N, D;
  const int32_t* task_var;    // [T] variable (block of bel)
  const int32_t* task_coord;  // [T] coordinate 0 .. D-1
  const int32_t* task_ptr;    // [T+1] CSR into task_rows
  const int32_t* task_rows;   // rows of `prop` whose marginal c enters task t
  const int32_t* task_joint;  // [T] 1: J[v][c] is the last density
  const double* prop;         // [rows][D][N]
  const double* prop_bw;      // [rows][D] or null: Silverman in-kernel
  const double* joint_bw;     // [V][D] or null: Silverman in-kernel
  double* bel;                // [V][D][N], in: J, out: the result
  uint32_t circ;              // bit c: coordinate c is an angle (differences and outputs wrapped)
  double inv_n, inv_nm1, c_n; // c_n: Silverman factor (4/(3N))^(1/5), host-computed
  uint64_t seed, stream_offset;
};

// LDS written by some lanes is read by others of the same wave: wave-level ordering is all that is needed
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int S>
__global__ void __launch_bounds__(64) k_product_coord(const CoordArgs a) {
  __shared__ double jl[64 * S];     // J[v][c][.], staged before the first store
  __shared__ double wts[64 * S];
  __shared__ double cumw[64 * S];
  const int t = blockIdx.x;
  if (t >= a.T) return;
  const int lane = threadIdx.x, N = a.N, D = a.D;
  const int v = a.task_var[t], c = a.task_coord[t], r0 = a.task_ptr[t], Mp = a.task_ptr[t + 1] - r0;
  if (Mp <= 0) return;              // (no partial row covers c: the coordinate keeps J)
  const bool joint = a.task_joint[t] != 0;
  const int M = Mp + (joint ? 1 : 0);
  const bool circ = ((a.circ >> c) & 1u) != 0u;
  double* ob = a.bel + ((size_t)v * D + c) * N;
  const double* __restrict__ prop = a.prop;
  auto line = [&](int l) { return prop + ((size_t)a.task_rows[r0 + l] * D + c) * N; };   // density l < Mp
  if (M == 1) {                     // one density: the output coordinate is that density, bit for bit
    const double* __restrict__ src = line(0);
    for (int i = lane; i < N; i += 64) ob[i] = src[i];
    return;
  }
  if (joint) {
#pragma unroll
    for (int s = 0; s < S; ++s) { const int i = lane + 64 * s; if (i < N) jl[i] = ob[i]; }
    wave_sync_lds();
  }
  // bandwidth of density l: supplied, or Silverman's rule on the spread about point 0; floored at 1e-6 either way
  auto bandwidth = [&](int l) {
    const bool is_j = l == Mp;
    const double* bw = is_j ? a.joint_bw : a.prop_bw;
    if (bw) return fmax(bw[is_j ? (size_t)v * D + c : (size_t)a.task_rows[r0 + l] * D + c], 1e-6);   // wave-uniform address
    const double* __restrict__ P = is_j ? nullptr : line(l);
    const double p0 = is_j ? jl[0] : P[0];
    double s[2] = {0.0, 0.0};
    for (int i = lane; i < N; i += 64) {
      const double e = (is_j ? jl[i] : P[i]) - p0, d = circ ? wrap_pi(e) : e;
      s[0] += d; s[1] += d * d;
    }
    wave_sum_n<2>(s);
    return fmax(a.c_n * fast_sqrt(fmax(0.0, (s[1] - s[0] * s[0] * a.inv_n) * a.inv_nm1)), 1e-6);
  };
  // pass 1: base = the density with the smallest bandwidth (ties to the lowest l), product bandwidth
  int base = 0;
  double best = __builtin_inf(), hp_acc = 0.0;
  for (int l = 0; l < M; ++l) {
    const double h = bandwidth(l), ih = 1.0 / h;
    hp_acc = fma(ih, ih, hp_acc);
    if (h < best) { best = h; base = l; }
  }
  const bool base_j = base == Mp;
  const double* __restrict__ Pb = base_j ? nullptr : line(base);
  // pass 2: log weights of the base points, densities in order
  double x[S], lw[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int i = lane + 64 * s, ii = i < N ? i : 0;
    x[s] = base_j ? jl[ii] : Pb[ii];
    lw[s] = 0.0;
  }
  for (int l = 0; l < M; ++l) {
    if (l == base) continue;
    const bool is_j = l == Mp;
    const double* __restrict__ P = is_j ? nullptr : line(l);
    const double ih = 1.0 / bandwidth(l);
    double qmin[S], sacc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) { qmin[s] = __builtin_inf(); sacc[s] = 0.0; }
    // one pass, running log-sum-exp: sacc = Σ_j exp(-½(q_j - qmin)) with qmin the smallest q seen so far
    for (int j = 0; j < N; ++j) {
      const double y = is_j ? jl[j] : P[j];   // wave-uniform address
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (lane + 64 * s < N) {              // skip idle slots (keeps exp() off them)
          const double e = x[s] - y, d = (circ ? wrap_pi(e) : e) * ih;
          const double q = d * d;
          const double dq = q - qmin[s];
          const double w = fast_exp_neg(-0.5 * fabs(dq));
          sacc[s] = dq < 0.0 ? fma(sacc[s], w, 1.0) : sacc[s] + w;
          qmin[s] = fmin(qmin[s], q);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) if (lane + 64 * s < N) lw[s] += -0.5 * qmin[s] + fast_log(sacc[s]);
  }
  // normalise, publish weights in point order
  double mx = -__builtin_inf();
#pragma unroll
  for (int s = 0; s < S; ++s) if (lane + 64 * s < N) mx = fmax(mx, lw[s]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
#pragma unroll
  for (int s = 0; s < S; ++s) { const int i = lane + 64 * s; if (i < N) wts[i] = exp(lw[s] - mx); }
  wave_sync_lds();
  // systematic resampling: cumulative weights by a sequential scan in point order (same arithmetic order as a CPU loop), then every
  // lane looks its picks up by bisection (first m with cum[m] > τ, else N-1)
  double cum = 0.0;
  for (int m = 0; m < N; ++m) {
    cum += wts[m];
    if (lane == (m & 63)) cumw[m] = cum;
  }
  wave_sync_lds();
  const double Tw = cumw[N - 1];
  const uint64_t stream = a.stream_offset + (uint64_t)v * (uint64_t)D + (uint64_t)c;
  const u32x4 uw = philox4x32_10(u32x4{0xFFFFFFFFu, (uint32_t)stream, (uint32_t)(stream >> 32), (3u << 16)},
                                 (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  const double u = ((double)uw.x + 0.5) * (1.0 / 4294967296.0);
  const double hp = 1.0 / fast_sqrt(hp_acc);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int i = lane + 64 * s;
    if (i < N) {
      const double tau = ((double)i + u) * Tw / (double)N;
      int lo = 0, hi = N - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cumw[mid] > tau) hi = mid; else lo = mid + 1;
      }
      double xi[1];
      rng_normals<1>(a.seed, stream, (uint32_t)i, xi);
      const double o = (base_j ? jl[lo] : Pb[lo]) + hp * xi[0];
      ob[i] = circ ? wrap_pi(o) : o;
    }
  }
}

hipError_t launch_product_partial(int dim, int T, int N, const int32_t* task_var, const int32_t* task_coord, const int32_t* task_ptr,
                                  const int32_t* task_rows, const int32_t* task_joint, const double* prop, const double* prop_bw,
                                  const double* joint_bw, uint32_t circ, double* bel, uint64_t seed, uint64_t stream_offset, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (N < 1 || N > kCoordMaxN || (dim != 2 && dim != 3 && dim != 6)) return hipErrorInvalidValue;
  CoordArgs a;
  a.T = T; a.N = N; a.D = dim; a.task_var = task_var; a.task_coord = task_coord; a.task_ptr = task_ptr; a.task_rows = task_rows;
  a.task_joint = task_joint; a.prop = prop; a.prop_bw = prop_bw; a.joint_bw = joint_bw; a.bel = bel; a.circ = circ;
  a.inv_n = 1.0 / N; a.inv_nm1 = N > 1 ? 1.0 / (N - 1) : 1.0; a.c_n = std::pow(4.0 / (3.0 * N), 0.2);
  a.seed = seed; a.stream_offset = stream_offset;
  const dim3 grid(T), block(64);
  if (N <= 64) hipLaunchKernelGGL((k_product_coord<1>), grid, block, 0, s, a);
  else if (N <= 128) hipLaunchKernelGGL((k_product_coord<2>), grid, block, 0, s, a);
  else if (N <= 256) hipLaunchKernelGGL((k_product_coord<4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_product_coord<8>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace rome
