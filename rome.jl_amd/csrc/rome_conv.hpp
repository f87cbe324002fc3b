// rome_conv.hpp -- batched factor-convolution kernels for gfx950 (MI355X): the kernel bodies and launch templates that every factor
// family shares.  A family's unit (rome_conv_pose2.hip, rome_conv_range.hip, rome_conv_pose3.hip, rome_conv_pose3_partial.hip) defines its policies, includes this
// header and instantiates the kernels through launch_solver<FP>.
//
// One convolution = approxConvBelief for one (factor, direction): N particle root-finds
// (IncrementalInference `computeAcrossHypothesis!` -> `_solveCCWNumeric!`)
// around the RoME residual functors (rows a2/a4/a6/a8).
//
// Two mappings:
//  * k_conv_flat -- the plain whole-graph sweep of a unique-root factor (closed form / Newton, in-kernel noise): the particles of
//    consecutive convolutions are PACKED onto the threads of a 256-thread block (thread = two neighbouring particles, 50 threads
//    per N = 100 convolution, 5 convolutions = 250 of 256 threads), per-factor μ / chol Σ staged through LDS.
//  * k_conv -- ONE WAVEFRONT PER CONVOLUTION for everything that needs a statistic over the N particles of a belief (the inflation
//    spread of the iterative solvers, multihypo / nullhypo) or pre-sampled noise.  Lane l owns particles 2l, 2l+1, 128+2l, ...
//    (PPL per lane, in registers), so
//   * the belief blocks are SoA [var][dim][N]: a wave reads/writes contiguous runs -> coalesced;
//   * per-factor constants (μ, chol Σ, var ids, direction) are wave-uniform -> scalar loads / SGPRs;
//   * the per-cycle belief statistics IIF needs for the entropy inflation (std of the N target
//     points) are pure wave64 xor-butterflies -- no LDS round trip, no __syncthreads();
//   * waves of a workgroup never wait for each other (Nelder-Mead trip counts differ per wave).
// Blocks are 256 threads = 4 convolutions; blockIdx is remapped so that each XCD (own L2) works on
// a contiguous range of the convolution table (neighbouring factors share variables).
#pragma once
#include <cstdlib>
#include <type_traits>
// Floating-point contraction by SOURCE EXPRESSION (a*b + c written in one expression is one fma), not across statements at the
// optimizer's discretion (hipcc's default, -ffp-contract=fast): the same inlined function then rounds identically in every kernel
// instantiation it is inlined into -- the packed sweep, the wave-per-row kernel (lean or not) and the per-factor entry points agree
// bit for bit for every solver (tests/test_gpu_config4.py), which "fast" does not guarantee.
#pragma clang fp contract(on)
#include "rome_device_math.hpp"
#include "rome_kernels.h"

namespace rome {

// block b runs on XCD b % 8 (observed dispatch rule; only used for L2 locality, never correctness).
__device__ __forceinline__ int xcd_contiguous_block(int b, int nb) {
  const int q = nb >> 3, r = nb & 7;
  const int xcd = b & 7, idx = b >> 3;
  return xcd * q + (xcd < r ? xcd : r) + idx;
}

// ---- belief statistics shared by the planar policies (Pose2 / Point2 targets of every family)
// std of the belief's tangent coordinates about particle 0 (shifted one-pass moments): SE(2)
template <int PPL>
__device__ __forceinline__ double spread_se2(const double (&t)[PPL][3], const bool (&act)[PPL], double inv, double den) {
  const double x0 = readlane_f64(t[0][0], 0), y0 = readlane_f64(t[0][1], 0), th0 = readlane_f64(t[0][2], 0);
  double s[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const double dx = t[k][0] - x0, dy = t[k][1] - y0, dt = wrap_pi(t[k][2] - th0);
    if (act[k]) { s[0] += dx; s[1] += dy; s[2] += dt; s[3] += dx * dx + dy * dy + dt * dt; }
  }
  // only the SUM of the coordinate variances is needed:  Σ_k var_k = (Σ_i |d_i|² − Σ_k (Σ_i d_ik)² / N) / (N − 1) -> four wave sums
  wave_sum_n<4>(s);
  const double v = fmax(0.0, (s[3] - (s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) * inv) * den);
  return fast_sqrt(v);   // Manifolds.std: root of the corrected Fréchet variance (sum of the coordinate variances)
}
template <int PPL>
__device__ __forceinline__ double spread_r2(const double (&t)[PPL][2], const bool (&act)[PPL], double inv, double den) {
  const double x0 = readlane_f64(t[0][0], 0), y0 = readlane_f64(t[0][1], 0);
  double s[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const double dx = t[k][0] - x0, dy = t[k][1] - y0;
    if (act[k]) { s[0] += dx; s[1] += dx * dx; s[2] += dy; s[3] += dy * dy; }
  }
  wave_sum_n<4>(s);
  const double vx = fmax(0.0, (s[1] - s[0] * s[0] * inv) * den);
  const double vy = fmax(0.0, (s[3] - s[2] * s[2] * inv) * den);
  return fast_sqrt(vx + vy);
}

// ------------------------------------------------------------------------------------------
// the convolution kernels
// ------------------------------------------------------------------------------------------
#ifndef ROME_P3_MINBLK
#define ROME_P3_MINBLK 1
#endif
#ifndef ROME_MIN_WAVES
#define ROME_MIN_WAVES 1
#endif
#ifndef ROME_NM_MINWAVES
#define ROME_NM_MINWAVES 4
#endif
#ifndef ROME_WPB
#define ROME_WPB 4   // wavefronts (= convolutions) per workgroup of k_conv
#endif

// slot k of lane `lane` -> particle: a lane owns NEIGHBOURING particles (2l, 2l+1), then (128 + 2l, 128 + 2l + 1), ...: the two
// particles that share a Box-Muller pair (rng_normals<3>) sit in one lane and are adjacent in every SoA row
template <int PPL>
__device__ __forceinline__ int slot_particle(int lane, int k) {
  if constexpr (PPL == 1) return lane;
  else return ((k >> 1) << 7) + 2 * lane + (k & 1);
}
// streaming (non-temporal) stores for data the launch does not read again
__device__ __forceinline__ void store_stream(double* p, double v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_stream2(double* p, const double2& v) {
  typedef double dvec2 __attribute__((ext_vector_type(2)));
  const dvec2 vv = {v.x, v.y};
  __builtin_nontemporal_store(vv, reinterpret_cast<dvec2*>(p));
}

// base + idx · stride_bytes + off_bytes for a NON-NEGATIVE index (row, block and factor indices are, by the table's contract) and a
// byte stride below 2^32: the product is one unsigned 32 x 32 -> 64 multiply-add (v_mad_u64_u32), exact for arrays of any size --
// written on int / size_t the same expression is a signed 64 x 64 partial product (v_mad_u64_u32 + 2 v_mul_lo_u32 + v_add3_u32 +
// v_ashrrev_i32 per site).  The packed sweep's launcher refuses strides that do not fit (launch_flat).
template <class T>
__device__ __forceinline__ T* row_ptr(T* base, int idx, uint32_t stride_bytes, uint32_t off_bytes = 0u) {
  typedef typename std::conditional<std::is_const<T>::value, const char, char>::type B;
  return reinterpret_cast<T*>(reinterpret_cast<B*>(base) + ((uint64_t)(uint32_t)idx * stride_bytes + off_bytes));
}

// separator rows are duplicated into the exchange buffer: block m of mirror_out for row c with mirror_map[c] = m >= 0
// (any number of rows), or -- the older form -- for the up to four rows listed in mirror_row
__device__ __forceinline__ int mirror_slot(const ConvArgs& a, int c_raw) {
  if (a.mirror_map) return a.mirror_map[c_raw];
  int m = -1;
  for (int q = 0; q < a.n_mirror; ++q) m = a.mirror_row[q] == c_raw ? q : m;
  return m;
}

template <class FP, int SOLVER, int PPL, bool LEAN> __device__ __forceinline__ void conv_wave_body(const ConvArgs& a, int blk);
// minimum waves / SIMD asked of the Nelder-Mead instantiations of k_conv (the 2-D / 3-D factors: see below).  The range factors'
// ring solve keeps its simplex in registers without that cap (capped at 128 VGPRs their PPL 4 / 8 kernels would spill): specialised in
// rome_conv_range.hip, before the first instantiation
template <class FP> struct NmMinWaves { static constexpr int value = ROME_NM_MINWAVES; };

// LEAN: the plain sweep -- in-kernel noise, all four table columns present, no multihypo / nullhypo rows.  The same code with
// those features compiled out: the table row is one 16-byte scalar load, nothing stands between the belief loads and the
// Philox / Box-Muller block, and the register allocation is not pinned by the feature paths.
template <class FP, int SOLVER, int PPL, bool LEAN>
// Nelder-Mead on the 2-D/3-D factors is latency-bound (long dependent select/compare chains): asking for 4 waves/SIMD
// (<= 128 VGPRs) is 5 % faster there; (the SE(3) kernels need their 256 VGPRs: capped at 3-4 waves/SIMD they spill and run 2.7x slower)
__global__ void __launch_bounds__(64 * ROME_WPB, (SOLVER == kSolverNelderMead && FP::DT <= 3) ? NmMinWaves<FP>::value : ((SOLVER != kSolverNelderMead && FP::DT == 6) ? ROME_P3_MINBLK : ROME_MIN_WAVES))
k_conv(const ConvArgs a) {
  conv_wave_body<FP, SOLVER, PPL, LEAN>(a, xcd_contiguous_block(blockIdx.x, gridDim.x));
}
template <class FP, int SOLVER, int PPL, bool LEAN>
__device__ __forceinline__ void conv_wave_body(const ConvArgs& a, int blk) {
  const int lane = threadIdx.x & 63;
  // no early exit: the (at most ROME_WPB - 1) surplus waves of the last block redo the last row and skip its stores, so that
  // no kernel-argument load has to wait for the n_conv comparison (all of them are issued together)
  const int c_raw = __builtin_amdgcn_readfirstlane(blk * ROME_WPB + (int)(threadIdx.x >> 6));
  const bool valid = c_raw < a.n_conv;
  const int c = valid ? c_raw : a.n_conv - 1;
  const int N = a.N;
  int f, dr, fv, tv;
  if (LEAN || a.rows4) {   // one 16-byte scalar load for the whole row
    const int4 row = *reinterpret_cast<const int4*>(a.rows4 + 4 * (size_t)c);
    f = row.x; fv = row.z; tv = row.w;
    dr = (FP::kHypoDir < 0 || FP::kHypoDir == 2) ? row.y : a.dir_all;   // bearing-range: the direction is the kernel's template argument
  } else {
    f = a.factor ? a.factor[c] : c;
    dr = a.dir ? a.dir[c] : a.dir_all;
    fv = a.fixed_var ? a.fixed_var[c] : c;
    tv = a.target_var ? a.target_var[c] : c;
  }
  const typename FP::Consts K = FP::load(a, f, dr);
  const double* __restrict__ fb = a.bel_fixed + (size_t)fv * FP::DF * N;
  const double* __restrict__ tb = a.bel_target + (size_t)tv * FP::DT * N;
  double* __restrict__ ob = a.out + (size_t)c * FP::DT * N;
  const uint64_t stream = a.stream_offset + (uint64_t)((!LEAN && a.row_stream) ? a.row_stream[c] : c);
  [[maybe_unused]] const int meas_blk = (!LEAN && a.meas_block) ? a.meas_block[c] : -1;

  double fx[PPL][FP::DF], t[PPL][FP::DT], z[PPL][FP::DZ];
  typename FP::Prep prep[PPL];
  typename FP::Aux aux[PPL];   // state a policy keeps beside the coordinates (Pose3: the rotation as a unit quaternion)
  bool act[PPL];
  [[maybe_unused]] double xi_odd[FP::DZ];   // normals of the odd slot, produced together with the even slot's (shared Philox calls)
  // measurement samples first (they depend on nothing but the convolution id), then the belief loads: the loaded particles
  // are then not live across the Philox / Box-Muller block (fewer registers at the kernel's pressure peak)
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const int i = slot_particle<PPL>(lane, k);
    act[k] = i < N;
    const int ii = act[k] ? i : 0;  // idle lanes shadow particle 0 (keeps the math finite, never stored)
    double xi[FP::DZ];
    if (!LEAN && meas_blk >= 0) {   // the row's measurement samples live in a belief block (a message of a child clique)
      const double* nb = a.meas_base + (size_t)meas_blk * FP::DZ * N;
#pragma unroll
      for (int d = 0; d < FP::DZ; ++d) xi[d] = nb[d * N + ii];
    } else if (!LEAN && a.noise) {
      const double* nb = a.noise + (size_t)c * FP::DZ * N;
#pragma unroll
      for (int d = 0; d < FP::DZ; ++d) xi[d] = nb[d * N + ii];
    } else if constexpr (PPL >= 2) {
      // slots k (even) and k+1 of a lane are the neighbours 2j, 2j+1: they draw from the same Philox calls (rng_normals_pair)
      if ((k & 1) == 0) rng_normals_pair<FP::DZ>(a.seed, stream, (uint32_t)i, xi, xi_odd);
      else {
#pragma unroll
        for (int d = 0; d < FP::DZ; ++d) xi[d] = xi_odd[d];
      }
    } else {
      rng_normals<FP::DZ>(a.seed, stream, (uint32_t)ii, xi);
    }
    if (!LEAN && ((a.noise && a.noise_is_meas) || meas_blk >= 0)) {   // the caller sampled the measurement model itself (any SamplableBelief)
#pragma unroll
      for (int d = 0; d < FP::DZ; ++d) z[k][d] = xi[d];
    } else FP::measurement(K, xi, z[k]);
  }
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const int i = slot_particle<PPL>(lane, k);
    const int ii = act[k] ? i : 0;
#pragma unroll
    for (int d = 0; d < FP::DF; ++d) fx[k][d] = fb[d * N + ii];
#pragma unroll
    for (int d = 0; d < FP::DT; ++d) t[k][d] = tb[d * N + ii];
    FP::canonical(t[k]);
    aux[k] = FP::init_aux(t[k]);
    prep[k] = FP::prepare(K, z[k], fx[k]);
  }

  int st[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) st[k] = 0;

  // ---- multihypo (IIF `multihypo=[1, w, 1-w]` on the second variable of a factor -- the landmark slot of a bearing-range
  //      factor, the second pose of a Pose2Pose2; ⚠IIF computeAcrossHypothesis!): per particle a categorical draw decides which
  //      candidate the measurement belongs to.
  //      side 1 (solve the first variable): the fixed particle comes from the drawn candidate.
  //      side 0 (solve this candidate): particles of the other hypothesis are not constrained by the factor: they keep
  //      their value and only receive entropy  spreadNH · ‖mean(this) - mean(other)‖ · (U-½)  (applied after the cycles).
  bool sel[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) sel[k] = true;
  double nh_spread = 0.0;
  [[maybe_unused]] int hd = FP::kHypoDir;   // which side of the factor is fractional (Pose2Pose2: by the row's direction)
  if constexpr (FP::kHypoDir >= 0 && !LEAN) {
    if constexpr (FP::kHypoDir == 2) hd = dr == 1 ? 1 : 0;
    const int av = (a.alt_var && dr != 2) ? a.alt_var[c] : -1;
    if (av >= 0) {  // wave-uniform
      const double w = a.hypo_w[c];
      const double* __restrict__ ab = (hd == 1 ? a.bel_fixed + (size_t)av * FP::DF * N : a.bel_target + (size_t)av * FP::DT * N);
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int i = slot_particle<PPL>(lane, k), ii = act[k] ? i : 0;
        const u32x4 hw = philox4x32_10(u32x4{(uint32_t)ii, (uint32_t)stream, (uint32_t)(stream >> 32), (4u << 16)},
                                       (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        const bool primary = ((double)hw.x + 0.5) * (1.0 / 4294967296.0) < w;
        if (hd == 1) {
          if (!primary) {
#pragma unroll
            for (int d = 0; d < FP::DF; ++d) fx[k][d] = ab[d * N + ii];
            prep[k] = FP::prepare(K, z[k], fx[k]);
          }
        } else sel[k] = primary;
      }
      if (hd == 0) {
        double sm[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < PPL; ++k) if (act[k]) {
          const int i = slot_particle<PPL>(lane, k);
          sm[0] += t[k][0]; sm[1] += t[k][1]; sm[2] += ab[i]; sm[3] += ab[N + i];
        }
        wave_sum_n<4>(sm);
        const double dx = (sm[0] - sm[2]) * a.inv_n, dy = (sm[1] - sm[3]) * a.inv_n;
        nh_spread = a.spread_nh * fast_sqrt(dx * dx + dy * dy);
      }
    }
  }

  // ---- nullhypo (IIF addFactor!(…, nullhypo=p), test/testPose3Pose3NH.jl:118): with probability p the factor does
  //      not apply to a particle; such particles keep their value and receive spreadNH · std entropy instead
  bool nullh[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) nullh[k] = false;
  double nh0_spread = 0.0;
  const double p_null = (!LEAN && a.nullhypo) ? a.nullhypo[c] : 0.0;
  if (p_null > 0.0) {  // wave-uniform
    const double sd0 = FP::template spread<PPL>(t, aux, act, a.inv_n, a.inv_nm1);
    nh0_spread = N > 1 ? a.spread_nh * (sd0 > 1e-10 ? sd0 : 1.0) : 0.0;   // calcStdBasicSpread fallback, as the inflation spread
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const uint32_t ii = (uint32_t)(act[k] ? slot_particle<PPL>(lane, k) : 0);
      const u32x4 w0 = philox4x32_10(u32x4{ii, (uint32_t)stream, (uint32_t)(stream >> 32), (5u << 16)}, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
      nullh[k] = ((double)w0.x + 0.5) * (1.0 / 4294967296.0) < p_null;   // (the entropy words are re-drawn after the cycles:
    }                                                                      //  nothing but this flag stays live across the solve)
  }

  // Inflation cycles (IIF inflateCycles x {addEntropyOnManifold!, N x solve}) apply where the start point can reach the answer: Nelder-Mead
  // everywhere, every solver on the bearing-range pose direction (a ring of roots); the jitter is drawn exactly as the oracle defines
  // it (ro_rng_entropy).  On a unique-root factor CLOSED_FORM / NEWTON return the root and GAUSS_NEWTON iterates to it from the belief
  // point: one pass, no statistic, no entropy.
  const bool cyc_on = FP::needs_cycles(SOLVER, K);
  const int ncyc = cyc_on ? (a.cycles < 1 ? 1 : a.cycles) : 1;
  for (int cyc = 0; cyc < ncyc; ++cyc) {
    double spread = 0.0;
    if (cyc_on && a.inflation > 0.0 && N > 1) {
#ifdef ROME_EXPERIMENT_NO_SPREAD   // experiment build (scripts/br1_bounds.py): no cross-particle statistic at all -- the bound on what
      const double sd = a.inv_n * (double)N * 0.02;   // packing rows / cheaper reductions could ever save (a run-time constant)
#else
      const double sd = FP::template spread<PPL>(t, aux, act, a.inv_n, a.inv_nm1);
#endif
      spread = a.inflation * (sd > 1e-10 ? sd : 1.0);   // IIF calcStdBasicSpread: "if no std yet, set to 1"
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (act[k] && sel[k] && !nullh[k]) {
        if (spread > 0.0) {
          double u[FP::DT];
#ifdef ROME_EXPERIMENT_NO_ENTROPY_RNG   // experiment build: the jitter without its Philox call (the bound on a cheaper generator)
#pragma unroll
          for (int d = 0; d < FP::DT; ++d) u[d] = 0.25 + 0.125 * (double)((lane + 3 * d + cyc) & 3);
#else
          rng_entropy_exact<FP::DT>(a.seed, stream, (uint32_t)slot_particle<PPL>(lane, k), cyc, u);
#endif
          FP::add_entropy(t[k], aux[k], spread, u);
        }
        st[k] = FP::template solve<SOLVER>(K, prep[k], z[k], fx[k], t[k], aux[k], a.max_iters, a.tol);
      }
    }
  }
  // NEWTON: the status is the residual FUNCTOR evaluated at the returned root (only when asked for)
  if constexpr (SOLVER == kSolverNewton) {
    if (a.status) {
#pragma unroll
      for (int k = 0; k < PPL; ++k)
        if (act[k] && sel[k] && !nullh[k]) st[k] = FP::verify(K, z[k], fx[k], t[k], aux[k], a.tol);
    }
  }

  if (p_null > 0.0 && nh0_spread > 0.0) {
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (act[k] && nullh[k]) {
        const uint32_t ii = (uint32_t)slot_particle<PPL>(lane, k);
        const u32x4 w0 = philox4x32_10(u32x4{ii, (uint32_t)stream, (uint32_t)(stream >> 32), (5u << 16)}, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        double u[FP::DT];
        const uint32_t e0[3] = {w0.y, w0.z, w0.w};
#pragma unroll
        for (int d = 0; d < (FP::DT < 3 ? FP::DT : 3); ++d) u[d] = ((double)e0[d] + 0.5) * (1.0 / 4294967296.0);
        if constexpr (FP::DT > 3) {
          const u32x4 w1 = philox4x32_10(u32x4{ii, (uint32_t)stream, (uint32_t)(stream >> 32), (5u << 16) | 1u}, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
          const uint32_t e1[3] = {w1.x, w1.y, w1.z};
#pragma unroll
          for (int d = 3; d < FP::DT; ++d) u[d] = ((double)e1[d - 3] + 0.5) * (1.0 / 4294967296.0);
        }
        FP::add_entropy(t[k], aux[k], nh0_spread, u);
      }
    }
  }
  if constexpr ((FP::kHypoDir == 0 || FP::kHypoDir == 2) && !LEAN) {
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (act[k] && !sel[k]) {  // the other hypothesis holds for this particle: entropy only
        // the words of the hypothesis draw are re-drawn here (same Philox call) instead of staying live across the cycles: kept in
        // per-slot arrays they were parked in LDS by the compiler
        const u32x4 hw = philox4x32_10(u32x4{(uint32_t)slot_particle<PPL>(lane, k), (uint32_t)stream, (uint32_t)(stream >> 32), (4u << 16)},
                                       (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        t[k][0] += nh_spread * (((double)hw.y + 0.5) * (1.0 / 4294967296.0) - 0.5);
        t[k][1] += nh_spread * (((double)hw.z + 0.5) * (1.0 / 4294967296.0) - 0.5);
        if constexpr (FP::DT == 3) t[k][2] = wrap_pi(t[k][2] + nh_spread * (((double)hw.w + 0.5) * (1.0 / 4294967296.0) - 0.5));   // a pose: the heading too, stored in (-π, π]
      }
    }
  }
  const int mslot = (a.n_mirror > 0 || a.mirror_map) ? mirror_slot(a, c_raw) : -1;   // wave-uniform
  double* mb = (mslot >= 0 && valid) ? a.mirror_out + (size_t)mslot * FP::DT * N : nullptr;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const int i = slot_particle<PPL>(lane, k);
    if (act[k] && valid) {
      FP::finalize(t[k], aux[k]);
#pragma unroll
      for (int d = 0; d < FP::DT; ++d) store_stream(ob + d * N + i, t[k][d]);   // (not read again by this launch: written through)
      if (a.status) a.status[(size_t)c * N + i] = st[k];
      if (mb) {
#pragma unroll
        for (int d = 0; d < FP::DT; ++d) store_stream(mb + d * N + i, t[k][d]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_conv_flat -- the plain sweep of a UNIQUE-ROOT factor (Pose2Pose2 + PriorPose2 rows, bearing-range -> landmark, Pose3Pose3) with
// CLOSED_FORM / NEWTON and in-kernel noise: nothing couples the particles of a convolution (no inflation statistic), so the
// particles of consecutive table rows are packed densely onto the threads of a block:
//   thread  = one PAIR of neighbouring particles (2j, 2j+1) of one row: the two share a Box-Muller pair (D = 3) and are adjacent
//             in every SoA row -> one 16-byte load / store per coordinate;
//   block   = CPB consecutive rows x H = ceil(N/2) pairs  (N = 100: 5 rows x 50 = 250 of 256 threads, against 100 of 128
//             lane-slots with one wavefront per row);
//   per-factor constants (μ, chol Σ) are staged ONCE per block through LDS: the first NK threads of every row load one entry each of
//             their own row's factor, every thread reads its row's slot back (broadcast reads); the table row itself is a 16-byte
//             load per thread.
// The root comes from FP::prepare (the same function the wave-per-row kernel and the per-factor entry points use: bit-identical
// proposals); NEWTON additionally evaluates the residual functor at the root when a status array is asked for.
// Any N >= 2; the start points u0 are never read (48 B of HBM traffic per Pose2 particle: fixed 24 + proposal 24).
// ------------------------------------------------------------------------------------------
constexpr int kFlatThreads = 256;
constexpr int kFlatMaxRows = 16;    // rows per block (rows of >= 8 pair-threads: N >= 16)
template <class FP> struct FlatStage { static constexpr int kLanes = FP::NK <= 16 ? 16 : 32; };   // LDS doubles per row (>= NK)

#ifndef ROME_FLAT_MINWAVES
#define ROME_FLAT_MINWAVES 8   // Pose2 / Point2 sweeps: 8 waves per SIMD (<= 64 VGPRs)
#endif
template <class FP, int SOLVER, bool VERIFY, bool VEC2, int PP>
__device__ __forceinline__ void conv_flat_body(const ConvArgs& a, int H, int CPB, uint32_t magic, int blk, double* __restrict__ s_K);
// entry q of factor f's staged constants [μ(DZ), L(NL)]: ONE address, selected between the two arrays before the entry offset is added
// (L is entered DZ entries before its start, so that q indexes both).  Integer arithmetic -- the address DZ entries before L is never
// formed as a pointer -- and an explicit global-memory load
template <class FP>
__device__ __forceinline__ double flat_stage_entry(const ConvArgs& a, int f, int q) {
  typedef const double __attribute__((address_space(1))) * GlobalPtr;
  const uint64_t pm = reinterpret_cast<uint64_t>(a.mu) + (uint64_t)(uint32_t)f * (8u * FP::DZ);
  const uint64_t pl = reinterpret_cast<uint64_t>(a.L) + (uint64_t)(uint32_t)f * (8u * FP::NL) - 8u * FP::DZ;
  return *reinterpret_cast<GlobalPtr>((q < FP::DZ ? pm : pl) + 8u * (uint32_t)q);
}
#ifndef ROME_FLAT_PP
#define ROME_FLAT_PP 1   // neighbouring particle pairs per thread of the packed sweep (Pose2 / Point2 factors).  Measured: 2 pairs per
                          // thread (fewer, fatter waves, one generation) need 96 VGPRs + spills and run 21.8 µs against 8.0 µs: one pair it is
#endif
#ifndef ROME_FLAT_GN_MINWAVES
#define ROME_FLAT_GN_MINWAVES 4   // the functor-iterating packed sweep (Pose2 / Point2): <= 128 VGPRs
#endif
#ifndef ROME_FLAT_GN6_MINWAVES
#define ROME_FLAT_GN6_MINWAVES 3   // SE(3) functor iteration on unit quaternions (round 6): asked to fit 168 VGPRs (three waves per SIMD, 7 spilled registers)
                                   // 85.4 us on the 10k helix against 88.4 us at 188 VGPRs / two waves; the sched barrier between a thread's two particles stays.
                                   // (round 5, 3x3 frames, profiles/r05_p3p3_gn_one_particle.txt: ONE particle per thread measured slower, 165.5 against 155.8 us.)
#endif
#ifndef ROME_FLAT_CF6_MINWAVES
#define ROME_FLAT_CF6_MINWAVES 1   // SE(3) closed form: 132 VGPRs (three waves per SIMD) 48.5 us on the 10k helix; pinned to 128 (four waves, 20 B of scratch) 49.7 us
#endif
template <class FP, int SOLVER, bool VERIFY, bool VEC2, int PP>
__global__ void __launch_bounds__(kFlatThreads, FP::DT <= 3 ? ((SOLVER == kSolverClosedForm && !VERIFY) ? (PP == 1 ? ROME_FLAT_MINWAVES : 5) : ROME_FLAT_GN_MINWAVES)
                                                            : (SOLVER == kSolverGaussNewton ? ROME_FLAT_GN6_MINWAVES : (VERIFY ? 1 : ROME_FLAT_CF6_MINWAVES)))
k_conv_flat(const ConvArgs a, int H, int CPB, uint32_t magic) {
  __shared__ double s_K[kFlatMaxRows * (FlatStage<FP>::kLanes + 2)];
  conv_flat_body<FP, SOLVER, VERIFY, VEC2, PP>(a, H, CPB, magic, xcd_contiguous_block(blockIdx.x, gridDim.x), s_K);
}
template <class FP, int SOLVER, bool VERIFY, bool VEC2, int PP>
__device__ __forceinline__ void conv_flat_body(const ConvArgs& a, int H, int CPB, uint32_t magic, int blk, double* __restrict__ s_K) {
  constexpr int SLP = FlatStage<FP>::kLanes + 2;   // (+2: rows of a wave's two convolutions start in different banks)
  constexpr int NP = 2 * PP;                        // particles per thread: PP neighbouring pairs (2·PP consecutive particles)
  const int tid = threadIdx.x;
#ifdef ROME_FLAT_TRACE   // experiment build (scripts/flat_trace.py): per-block timestamps instead of the status array
  const uint64_t trace_t0 = wall_clock64();
#endif
  const int c0 = blk * CPB;
  const int N = a.N;
  // ---- this thread's (row, particle group)
  const int lc_raw = (int)(((uint32_t)tid * magic) >> 16);   // tid / H
  const int j = tid - lc_raw * H;
  const bool live = lc_raw < CPB && c0 + lc_raw < a.n_conv;
  const int lc = lc_raw < CPB ? lc_raw : CPB - 1;
  const int c = min(c0 + lc, a.n_conv - 1);
  const int4 row = *row_ptr(reinterpret_cast<const int4*>(a.rows4), c, 16u);
  const int dr = (FP::kHypoDir < 0 || FP::kHypoDir == 2) ? row.y : a.dir_all;
  const int i0 = NP * j;                      // particles i0 .. i0 + NP - 1 (the tail of a row may be shorter)
  const uint32_t sN = 8u * (uint32_t)N;       // byte strides: one coordinate, one block of the fixed / the target belief (uniform)
  const uint32_t sF = (uint32_t)FP::DF * sN, sT = (uint32_t)FP::DT * sN;
  // ---- per-factor constants -> LDS: the first threads of every row load one entry each of THEIR OWN row's factor (the factor
  //      index arrives with the row they need anyway: the load is issued beside the belief loads, nothing waits for it here;
  //      branch-free: every thread loads SOME valid entry, only the first NK of a row publish theirs)
  constexpr int KP = (FP::NK + 7) / 8;   // passes (H >= 8 threads per row); pass e serves entries [e·H, (e + 1)·H): with H >= NK / e
  double kst[KP];                         // it has none, and the whole block skips it (H is uniform; the first pass always runs)
  kst[0] = flat_stage_entry<FP>(a, row.x, min(j, FP::NK - 1));
  // the fixed belief's block, entered at this thread's first particle (idle threads shadow particle 0): coordinate d lies d·N doubles on
  double fx[NP][FP::DF];
  [[maybe_unused]] double t0[NP][FP::DT];   // GAUSS_NEWTON: the start points u0 (the target's current belief): +24 B per Pose2 particle
#pragma unroll
  for (int p = 0; p < PP; ++p) {
    const int ip = i0 + 2 * p;
    const uint32_t o0 = 8u * (uint32_t)(ip < N ? ip : 0), o1 = 8u * (uint32_t)(ip + 1 < N ? ip + 1 : 0);
    if (VEC2) {   // (N even: a pair is inside the row or entirely beyond it)
      const double* __restrict__ fb = row_ptr(a.bel_fixed, row.z, sF, o0);
#pragma unroll
      for (int d = 0; d < FP::DF; ++d) {
        const double2 v = *reinterpret_cast<const double2*>(fb + (size_t)d * N);
        fx[2 * p][d] = v.x; fx[2 * p + 1][d] = v.y;
      }
    } else {
      const double* __restrict__ fb0 = row_ptr(a.bel_fixed, row.z, sF, o0);
      const double* __restrict__ fb1 = row_ptr(a.bel_fixed, row.z, sF, o1);
#pragma unroll
      for (int d = 0; d < FP::DF; ++d) { fx[2 * p][d] = fb0[(size_t)d * N]; fx[2 * p + 1][d] = fb1[(size_t)d * N]; }
    }
    if constexpr (SOLVER == kSolverGaussNewton) {
      const double* __restrict__ tb0 = row_ptr(a.bel_target, row.w, sT, o0);
      const double* __restrict__ tb1 = row_ptr(a.bel_target, row.w, sT, o1);
#pragma unroll
      for (int d = 0; d < FP::DT; ++d) { t0[2 * p][d] = tb0[(size_t)d * N]; t0[2 * p + 1][d] = tb1[(size_t)d * N]; }
    }
  }
#pragma unroll
  for (int e = 1; e < KP; ++e) kst[e] = e * H < FP::NK ? flat_stage_entry<FP>(a, row.x, min(j + e * H, FP::NK - 1)) : 0.0;   // (behind the belief loads: the branch splits no load group)
  // ---- measurement noise (depends on the row id only).  The two compiler fences keep the order {loads issued} -> {Philox /
  //      Box-Muller} -> {first use of a loaded value}, so that the generator runs under the load latency (left alone, the
  //      compiler sinks the generator below the LDS write and its s_waitcnt vmcnt(0))
  asm volatile("" ::: "memory");
  const uint64_t stream = a.stream_offset + (uint64_t)(uint32_t)c;   // (c >= 0: zero extension, the same counter)
  double xi[NP][FP::DZ];
#pragma unroll
  for (int p = 0; p < PP; ++p) rng_normals_pair<FP::DZ>(a.seed, stream, (uint32_t)(i0 + 2 * p), xi[2 * p], xi[2 * p + 1]);
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int d = 0; d < FP::DZ; ++d) asm volatile("" : "+v"(xi[k][d]) :: "memory");
  }
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    const int q = j + e * H;
    if (e > 0 && e * H >= FP::NK) continue;
    if (lc_raw < CPB && q < FP::NK) s_K[lc * SLP + q] = kst[e];
  }
  __syncthreads();
  const typename FP::Consts K = FP::from_lds(s_K + lc * SLP, dr);
  double t[NP][FP::DT];
  int st[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    double z[FP::DZ];
    st[k] = 0;
    FP::measurement(K, xi[k], z);
    const typename FP::Prep P = FP::prepare(K, z, fx[k]);
    if constexpr (SOLVER == kSolverGaussNewton) {   // the numerical root-find on the residual functor, from the belief point
      // SE(3): one particle's iteration holds two 3x3 frames, Exp(z_ω), the update and the residual (~110 VGPRs): the two particles of
      // a thread run one AFTER the other (no interleaving across this point), or the allocation doubles and one wave per SIMD is left
      if constexpr (FP::DT == 6) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int d = 0; d < FP::DT; ++d) t[k][d] = t0[k][d];
      FP::canonical(t[k]);
      typename FP::Aux A = FP::init_aux(t[k]);
      st[k] = FP::template solve<kSolverGaussNewton>(K, P, z, fx[k], t[k], A, a.max_iters, a.tol);
      FP::finalize(t[k], A);
    } else {
      typename FP::Aux A;
      FP::template solve<kSolverClosedForm>(K, P, z, fx[k], t[k], A, 0, 0.0);
      if constexpr (VERIFY) st[k] = FP::verify(K, z, fx[k], t[k], A, a.tol);   // NEWTON with a status array: the functor at the root
      FP::finalize(t[k], A);
    }
  }
#ifdef ROME_FLAT_TRACE
  const uint64_t trace_t1 = wall_clock64();
#endif
  if (!live) return;
  const int mslot = (a.n_mirror > 0 || a.mirror_map) ? mirror_slot(a, c) : -1;
#pragma unroll
  for (int p = 0; p < PP; ++p) {
    const int ip = i0 + 2 * p;
    if (ip >= N) continue;
    const bool act1 = ip + 1 < N;               // (odd N: the last pair is a single particle)
    double* __restrict__ ob = row_ptr(a.out, c, sT, 8u * (uint32_t)ip);
    double* mb = mslot >= 0 ? row_ptr(a.mirror_out, mslot, sT, 8u * (uint32_t)ip) : nullptr;
    if (VEC2) {
#pragma unroll
      for (int d = 0; d < FP::DT; ++d) {
        const double2 v = {t[2 * p][d], t[2 * p + 1][d]};
        // streaming stores: the proposals are not read again by this launch; written through, they are not left dirty in the L2
        // for the end-of-kernel write-back (measured: 9.1 -> 7.8 µs per Manhattan sweep)
        store_stream2(ob + (size_t)d * N, v);
        if (mb) store_stream2(mb + (size_t)d * N, v);
      }
    } else {
#pragma unroll
      for (int d = 0; d < FP::DT; ++d) {
        store_stream(ob + (size_t)d * N, t[2 * p][d]); if (act1) store_stream(ob + (size_t)d * N + 1, t[2 * p + 1][d]);
        if (mb) { store_stream(mb + (size_t)d * N, t[2 * p][d]); if (act1) store_stream(mb + (size_t)d * N + 1, t[2 * p + 1][d]); }
      }
    }
#ifndef ROME_FLAT_TRACE
    if (a.status) { int* sb = row_ptr(a.status, c, 4u * (uint32_t)N, 4u * (uint32_t)ip); sb[0] = st[2 * p]; if (act1) sb[1] = st[2 * p + 1]; }
#endif
  }
#ifdef ROME_FLAT_TRACE
  if (a.status && tid == 0) {
    uint64_t* tr = reinterpret_cast<uint64_t*>(a.status) + 4 * (size_t)blockIdx.x;
    tr[0] = trace_t0; tr[1] = trace_t1; tr[2] = wall_clock64();
    tr[3] = (uint64_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) | ((uint64_t)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32);   // HW_ID, XCC_ID
  }
#endif
}

// ------------------------------------------------------------------------------------------
// N > 512: the same convolution with the particles walked in chunks of 128 instead of living in registers for the whole
// kernel.  Cycle by cycle: (1) the spread of ALL N current points (the start points u0 in cycle 0, the previous cycle's
// solutions afterwards -- they are re-read from the proposal block itself), (2) chunk by chunk: load, re-draw the measurement
// samples (counter-based: the same every time), jitter with the oracle's uniforms, solve, store.  One wavefront per convolution; multihypo / nullhypo rows are not served here (the launcher refuses them).
// ------------------------------------------------------------------------------------------
template <class FP, int SOLVER>
__global__ void __launch_bounds__(64 * ROME_WPB) k_conv_big(const ConvArgs a) {
  constexpr int PPL = 2;
  const int lane = threadIdx.x & 63;
  const int c_raw = __builtin_amdgcn_readfirstlane(xcd_contiguous_block(blockIdx.x, gridDim.x) * ROME_WPB + (int)(threadIdx.x >> 6));
  const bool valid = c_raw < a.n_conv;
  const int c = valid ? c_raw : a.n_conv - 1;
  const int N = a.N;
  int f, dr, fv, tv;
  if (a.rows4) {
    const int4 row = *reinterpret_cast<const int4*>(a.rows4 + 4 * (size_t)c);
    f = row.x; fv = row.z; tv = row.w; dr = (FP::kHypoDir < 0 || FP::kHypoDir == 2) ? row.y : a.dir_all;
  } else {
    f = a.factor ? a.factor[c] : c; dr = a.dir ? a.dir[c] : a.dir_all;
    fv = a.fixed_var ? a.fixed_var[c] : c; tv = a.target_var ? a.target_var[c] : c;
  }
  const typename FP::Consts K = FP::load(a, f, dr);
  const double* __restrict__ fb = a.bel_fixed + (size_t)fv * FP::DF * N;
  const double* tb = a.bel_target + (size_t)tv * FP::DT * N;
  double* ob = a.out + (size_t)c * FP::DT * N;
  const uint64_t stream = a.stream_offset + (uint64_t)(a.row_stream ? a.row_stream[c] : c);
  const int meas_blk = a.meas_block ? a.meas_block[c] : -1;
  const bool cyc_on = FP::needs_cycles(SOLVER, K);
  const int ncyc = cyc_on ? (a.cycles < 1 ? 1 : a.cycles) : 1;
  if (!valid) return;   // (nothing below synchronises across waves; surplus waves of the last block have no row)
  for (int cyc = 0; cyc < ncyc; ++cyc) {
    const double* cur = cyc == 0 ? tb : ob;
    double spread = 0.0;
    if (cyc_on && a.inflation > 0.0 && N > 1) {
      double t0[FP::DT];
#pragma unroll
      for (int d = 0; d < FP::DT; ++d) t0[d] = cur[d * N];
      FP::canonical(t0);
      const typename FP::Aux a0 = FP::init_aux(t0);
      const typename FP::Ref ref = FP::make_ref(t0, a0);
      double sm[2 * FP::DT];
#pragma unroll
      for (int j = 0; j < 2 * FP::DT; ++j) sm[j] = 0.0;
      for (int i = lane; i < N; i += 64) {
        double t[FP::DT], dd[FP::DT];
#pragma unroll
        for (int d = 0; d < FP::DT; ++d) t[d] = cur[d * N + i];
        FP::canonical(t);
        const typename FP::Aux ax = FP::init_aux(t);
        FP::tangent(ref, t, ax, dd);
#pragma unroll
        for (int d = 0; d < FP::DT; ++d) { sm[2 * d] += dd[d]; sm[2 * d + 1] += dd[d] * dd[d]; }
      }
      wave_sum_n<2 * FP::DT>(sm);
      double var = 0.0;
#pragma unroll
      for (int d = 0; d < FP::DT; ++d) var += fmax(0.0, (sm[2 * d + 1] - sm[2 * d] * sm[2 * d] * a.inv_n) * a.inv_nm1);
      const double sd = fast_sqrt(var);
      spread = a.inflation * (sd > 1e-10 ? sd : 1.0);
    }
    for (int base = 0; base < N; base += 64 * PPL) {
      double fx[PPL][FP::DF], t[PPL][FP::DT], z[PPL][FP::DZ];
      typename FP::Aux aux[PPL];
      bool act[PPL];
      [[maybe_unused]] double xi_odd[FP::DZ];
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int i = base + 2 * lane + k;
        act[k] = i < N;
        const int ii = act[k] ? i : 0;
#pragma unroll
        for (int d = 0; d < FP::DF; ++d) fx[k][d] = fb[d * N + ii];
#pragma unroll
        for (int d = 0; d < FP::DT; ++d) t[k][d] = cur[d * N + ii];
        double xi[FP::DZ];
        if (meas_blk >= 0) {
          const double* nb = a.meas_base + (size_t)meas_blk * FP::DZ * N;
#pragma unroll
          for (int d = 0; d < FP::DZ; ++d) xi[d] = nb[d * N + ii];
        } else if (a.noise) {
          const double* nb = a.noise + (size_t)c * FP::DZ * N;
#pragma unroll
          for (int d = 0; d < FP::DZ; ++d) xi[d] = nb[d * N + ii];
        } else {   // the neighbours 2j, 2j+1 draw from the same Philox calls (rng_normals_pair)
          if ((k & 1) == 0) rng_normals_pair<FP::DZ>(a.seed, stream, (uint32_t)i, xi, xi_odd);
          else {
#pragma unroll
            for (int d = 0; d < FP::DZ; ++d) xi[d] = xi_odd[d];
          }
        }
        if ((a.noise && a.noise_is_meas) || meas_blk >= 0) {
#pragma unroll
          for (int d = 0; d < FP::DZ; ++d) z[k][d] = xi[d];
        } else FP::measurement(K, xi, z[k]);
        FP::canonical(t[k]);
        aux[k] = FP::init_aux(t[k]);
      }
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int i = base + 2 * lane + k;
        if (act[k]) {
          const typename FP::Prep prep = FP::prepare(K, z[k], fx[k]);
          if (spread > 0.0) {
            double u[FP::DT];
            rng_entropy_exact<FP::DT>(a.seed, stream, (uint32_t)i, cyc, u);
            FP::add_entropy(t[k], aux[k], spread, u);
          }
          int st = FP::template solve<SOLVER>(K, prep, z[k], fx[k], t[k], aux[k], a.max_iters, a.tol);
          if constexpr (SOLVER == kSolverNewton) { if (a.status) st = FP::verify(K, z[k], fx[k], t[k], aux[k], a.tol); }
          FP::finalize(t[k], aux[k]);
#pragma unroll
          for (int d = 0; d < FP::DT; ++d) ob[d * N + i] = t[k][d];
          if (a.status) a.status[(size_t)c * N + i] = st;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the next cycle's spread pass reads what other lanes of this wave just wrote
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
}

// ------------------------------------------------------------------------------------------
// k_deconv -- approxDeconv of a table of relative factors: for row c = (factor, var_a, var_b), particle i of the first variable is
// paired with particle i of the second, and
//   pred[c][.][i] = FP::predict(a_i, b_i)   the measurement (tangent coordinates) at which the factor's residual vanishes on the pair;
//   meas[c][.][i] = what the convolution of row c draws for particle i: FP::measurement on the normals of (seed, stream_offset + c, i)
//                   (rng_normals: the counter is the particle id, so the draw is the one rng_normals_pair hands the sweeps), or on
//                   the caller's noise rows, or those rows themselves (noise_is_meas).
// PRED / MEAS are compiled in or out (either output may be absent).  thread = one particle of one row: the reads run along N in the SoA
// blocks.  Rows of fewer than 256 particles are packed RPB = 256 / N to a block (N = 100: two rows, 200 of 256 threads; at most 16),
// longer rows are cut into chunks of 256 along gridDim.y.  The constants [μ(DZ), L(NL)] of a block's rows are staged once per row
// through LDS by the block's threads (one entry each).  FP is a policy in its dir-0 form: DF / DT are the dimensions of the factor's
// first / second variable.  No atomics, nothing is shared between rows but the staging barrier: the bits of row c depend on row c alone.
// ------------------------------------------------------------------------------------------
constexpr int kDeconvThreads = 256;
constexpr int kDeconvMaxRows = 16;

// the Pose2Pose2 measurement of two SE(2) points: R_pᵀ (t_q − t_p) and the angle of R_pᵀ R_q, read as residual_pose2pose2 reads its own
__device__ __forceinline__ void predict_se2(const Se2& P, const Se2& Q, double (&z)[3]) {
  const double dx = Q.x - P.x, dy = Q.y - P.y;
  z[0] = P.c * dx + P.s * dy;
  z[1] = P.c * dy - P.s * dx;
  const double U11 = P.c * Q.c + P.s * Q.s, U21 = P.c * Q.s - P.s * Q.c;
  z[2] = fast_atan2(U21, U11);
}

template <class FP, bool PRED, bool MEAS>
__global__ void __launch_bounds__(kDeconvThreads) k_deconv(const DeconvArgs a, int H, int RPB, uint32_t magic) {
  static_assert(PRED || MEAS, "an output");
  static_assert(FP::NK == FP::DZ + FP::NL, "the staged image is [mu, L]");
  constexpr int SLP = FP::NK | 1;   // (odd: the rows of a block start in different banks)
  __shared__ double s_K[MEAS ? kDeconvMaxRows * SLP : 1];
  const int tid = threadIdx.x;
  const int N = a.N;
  const int c0 = blockIdx.x * RPB;
  // ---- this thread's (row, particle): idle threads shadow the block's last row / particle 0 and store nothing
  const int lr_raw = (int)(((uint32_t)tid * magic) >> 16);   // tid / H
  const int j = tid - lr_raw * H;
  const int i = (int)blockIdx.y * kDeconvThreads + j;
  const bool live = lr_raw < RPB && c0 + lr_raw < a.n_rows && i < N;
  const int lr = lr_raw < RPB ? lr_raw : RPB - 1;
  const int c = min(c0 + lr, a.n_rows - 1);
  const int ii = i < N ? i : 0;
  [[maybe_unused]] int va, vb;
  if (a.rows4) {
    const int4 row = *row_ptr(reinterpret_cast<const int4*>(a.rows4), c, 16u);
    va = row.z; vb = row.w;
  } else {
    va = a.var_a ? a.var_a[c] : c;
    vb = a.var_b ? a.var_b[c] : c;
  }
  if constexpr (MEAS) {
    const bool given = a.noise != nullptr && a.noise_is_meas != 0;   // (uniform) the rows ARE the samples: no constants are read
    if (!given) {
      for (int e = tid; e < RPB * FP::NK; e += kDeconvThreads) {
        const int r = e / FP::NK, q = e - r * FP::NK;
        const int cr = min(c0 + r, a.n_rows - 1);
        const int fr = a.rows4 ? a.rows4[4 * (size_t)cr] : (a.factor ? a.factor[cr] : cr);
        s_K[r * SLP + q] = q < FP::DZ ? a.mu[(size_t)fr * FP::DZ + q] : a.L[(size_t)fr * FP::NL + (q - FP::DZ)];
      }
    }
    double xi[FP::DZ], z[FP::DZ];
    if (a.noise) {
      const double* __restrict__ nb = a.noise + (size_t)c * FP::DZ * N;
#pragma unroll
      for (int d = 0; d < FP::DZ; ++d) xi[d] = nb[(size_t)d * N + ii];
    } else {
      rng_normals<FP::DZ>(a.seed, a.stream_offset + (uint64_t)(uint32_t)c, (uint32_t)ii, xi);
    }
    __syncthreads();
    if (given) {
#pragma unroll
      for (int d = 0; d < FP::DZ; ++d) z[d] = xi[d];
    } else {
      const typename FP::Consts K = FP::from_lds(s_K + lr * SLP, 0);
      FP::measurement(K, xi, z);
    }
    if (live) {
      double* __restrict__ mb = a.meas + (size_t)c * FP::DZ * N;
#pragma unroll
      for (int d = 0; d < FP::DZ; ++d) mb[(size_t)d * N + i] = z[d];
    }
  }
  if constexpr (PRED) {
    const double* __restrict__ ab = a.bel_a + (size_t)va * FP::DF * N;
    const double* __restrict__ bb = a.bel_b + (size_t)vb * FP::DT * N;
    double pa[FP::DF], pb[FP::DT], z[FP::DZ];
#pragma unroll
    for (int d = 0; d < FP::DF; ++d) pa[d] = ab[(size_t)d * N + ii];
#pragma unroll
    for (int d = 0; d < FP::DT; ++d) pb[d] = bb[(size_t)d * N + ii];
    FP::predict(pa, pb, z);
    if (live) {
      double* __restrict__ pr = a.pred + (size_t)c * FP::DZ * N;
#pragma unroll
      for (int d = 0; d < FP::DZ; ++d) pr[(size_t)d * N + i] = z[d];
    }
  }
}

template <class FP>
static hipError_t launch_deconv_t(const DeconvArgs& a, hipStream_t s) {
  if (a.n_rows <= 0) return hipSuccess;
  if (a.N < 1 || (!a.pred && !a.meas)) return hipErrorInvalidValue;
  const int H = a.N < kDeconvThreads ? a.N : kDeconvThreads;
  int RPB = kDeconvThreads / H;
  if (RPB > kDeconvMaxRows) RPB = kDeconvMaxRows;
  const uint32_t magic = (65536u + (uint32_t)H - 1u) / (uint32_t)H;   // tid / H == (tid * magic) >> 16 for tid < 256 (checked below)
  for (int t = 0; t < kDeconvThreads; ++t) if ((int)(((uint32_t)t * magic) >> 16) != t / H) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.n_rows + RPB - 1) / RPB), (unsigned)((a.N + kDeconvThreads - 1) / kDeconvThreads));
  if (a.pred && a.meas) hipLaunchKernelGGL((k_deconv<FP, true, true>), grid, dim3(kDeconvThreads), 0, s, a, H, RPB, magic);
  else if (a.pred)      hipLaunchKernelGGL((k_deconv<FP, true, false>), grid, dim3(kDeconvThreads), 0, s, a, H, RPB, magic);
  else                  hipLaunchKernelGGL((k_deconv<FP, false, true>), grid, dim3(kDeconvThreads), 0, s, a, H, RPB, magic);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <class FP, int SOLVER, bool LEAN>
static hipError_t launch_ppl_v(const ConvArgs& a, hipStream_t s) {
  const int nb = (a.n_conv + ROME_WPB - 1) / ROME_WPB;
  if (nb == 0) return hipSuccess;
  if (a.N <= 64)       hipLaunchKernelGGL((k_conv<FP, SOLVER, 1, LEAN>), dim3(nb), dim3(64 * ROME_WPB), 0, s, a);
  else if (a.N <= 128) hipLaunchKernelGGL((k_conv<FP, SOLVER, 2, LEAN>), dim3(nb), dim3(64 * ROME_WPB), 0, s, a);
  else if (a.N <= 256) hipLaunchKernelGGL((k_conv<FP, SOLVER, 4, LEAN>), dim3(nb), dim3(64 * ROME_WPB), 0, s, a);
  else if (a.N <= 512) hipLaunchKernelGGL((k_conv<FP, SOLVER, 8, LEAN>), dim3(nb), dim3(64 * ROME_WPB), 0, s, a);
  else {   // particles walked in chunks (k_conv_big); rows with multihypo / nullhypo / mirrors stay on the register-resident kernels
    if (a.alt_var || a.nullhypo || a.n_mirror > 0 || a.mirror_map) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_conv_big<FP, SOLVER>), dim3(nb), dim3(64 * ROME_WPB), 0, s, a);
  }
  return hipGetLastError();
}
// the packed sweep (k_conv_flat): H = ceil(N/2) pair-threads per row, CPB rows per 256-thread block
template <class FP, int SOLVER>
static hipError_t launch_flat(const ConvArgs& a, hipStream_t s) {
  // PP neighbouring pairs per thread: Pose2 / Point2 rows of >= 64 particles take ROME_FLAT_PP, everything else one pair
  constexpr int PPC = FP::DT <= 3 ? ROME_FLAT_PP : 1;
  const bool verify = SOLVER == kSolverNewton && a.status != nullptr;
  const int pp = (PPC > 1 && a.N >= 64 && !verify && SOLVER != kSolverGaussNewton) ? PPC : 1;
  const int H = (a.N + 2 * pp - 1) / (2 * pp);
  int CPB = kFlatThreads / H;
  if (CPB > kFlatMaxRows) CPB = kFlatMaxRows;
  const uint32_t magic = (65536u + (uint32_t)H - 1u) / (uint32_t)H;   // tid / H == (tid * magic) >> 16 for tid < 256 (checked below)
  for (int t = 0; t < kFlatThreads; ++t) if ((int)(((uint32_t)t * magic) >> 16) != t / H) return hipErrorInvalidValue;
  const int nb = (a.n_conv + CPB - 1) / CPB;
  if (nb == 0) return hipSuccess;
  // the kernel forms a row's address as index x byte stride in 32 x 32 -> 64 bits (row_ptr): one block of either belief has to span
  // less than 2^32 bytes (always, at the N <= 512 this launch is reached with)
  if ((uint64_t)(FP::DF > FP::DT ? FP::DF : FP::DT) * 8u * (uint64_t)a.N > 0xFFFFFFFFull) return hipErrorInvalidValue;
  // 16-byte accesses need an even N (row starts stay 16-byte aligned) and 16-byte aligned arrays
  const bool vec2 = (a.N % 2 == 0) && (((uintptr_t)a.bel_fixed | (uintptr_t)a.out | (uintptr_t)a.mirror_out) % 16 == 0);
  // (the functor evaluation is a separate instantiation: compiled into the plain sweep it would pin its register allocation)
  constexpr int CF = kSolverClosedForm, GN = kSolverGaussNewton;
  if constexpr (SOLVER == kSolverGaussNewton) {   // the functor-iterating packed sweep
    if (vec2) hipLaunchKernelGGL((k_conv_flat<FP, GN, false, true, 1>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
    else      hipLaunchKernelGGL((k_conv_flat<FP, GN, false, false, 1>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
  } else if (verify) {
    if (vec2) hipLaunchKernelGGL((k_conv_flat<FP, CF, true, true, 1>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
    else      hipLaunchKernelGGL((k_conv_flat<FP, CF, true, false, 1>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
  } else if (pp == 1) {
    if (vec2) hipLaunchKernelGGL((k_conv_flat<FP, CF, false, true, 1>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
    else      hipLaunchKernelGGL((k_conv_flat<FP, CF, false, false, 1>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
  } else {
    if (vec2) hipLaunchKernelGGL((k_conv_flat<FP, CF, false, true, PPC>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
    else      hipLaunchKernelGGL((k_conv_flat<FP, CF, false, false, PPC>), dim3(nb), dim3(kFlatThreads), 0, s, a, H, CPB, magic);
  }
  return hipGetLastError();
}
template <class FP, int SOLVER>
static hipError_t launch_ppl(const ConvArgs& a, hipStream_t s) {
  const bool lean = a.rows4 != nullptr && a.noise == nullptr && a.alt_var == nullptr && a.nullhypo == nullptr && a.row_stream == nullptr &&
                    a.meas_block == nullptr;
  if constexpr (FP::kUniqueRoot && (SOLVER == kSolverClosedForm || SOLVER == kSolverNewton || SOLVER == kSolverGaussNewton)) {
    // plain sweep of a unique-root factor: the packed kernel (rows of >= 8 pair-threads; tiny N stays one wavefront per row) -- the
    // analytic root, or the Gauss-Newton iteration on the residual functor from the belief point (nothing couples the particles of a
    // row either way: no inflation statistic)
    if (lean && a.N >= 16 && (a.N + 1) / 2 <= kFlatThreads) return launch_flat<FP, SOLVER>(a, s);
  }
  // NEWTON without a status array IS the closed form on every factor here (unique roots; the bearing-range pose direction steps
  // exactly onto the ring member its start selects): one instantiation (the functor evaluation of the status path would otherwise
  // pin the register allocation of the plain launch)
  if constexpr (SOLVER == kSolverNewton) { if (!a.status) return launch_ppl<FP, kSolverClosedForm>(a, s); }
  return lean ? launch_ppl_v<FP, SOLVER, true>(a, s) : launch_ppl_v<FP, SOLVER, false>(a, s);
}
template <class FP>
static hipError_t launch_solver(const ConvArgs& a, int solver, hipStream_t s) {
  switch (solver) {
    case kSolverClosedForm:  return launch_ppl<FP, kSolverClosedForm>(a, s);
    case kSolverNewton:      return launch_ppl<FP, kSolverNewton>(a, s);
    case kSolverNelderMead:  return launch_ppl<FP, kSolverNelderMead>(a, s);
    case kSolverGaussNewton: return launch_ppl<FP, kSolverGaussNewton>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace rome
