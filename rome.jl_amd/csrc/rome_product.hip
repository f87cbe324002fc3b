// rome_product.hip -- belief statistics and the proposal product.
//
//  * k_belief_stats<D>: manifold mean + per-coordinate std of every belief (N particles), the PPE-style summary
//    (`getPPE(...).suggested`, examples/ManhattanBatchAnalysis.jl:59-62) and the input of the KDE bandwidths;
//    same definition as the inflation spread (tangent coordinates about particle 0).
//  * k_product<M,S>: new belief of a variable from its K proposals -- a regularised importance-sampling product
//    of the K kernel density estimates.  This is a STAND-IN for ApproxManifoldProducts.manifoldProduct
//    (unvendored multiscale Gibbs product): the definition is the one in
//    oracle/rome_oracle.c (ro_product, ro_product_bw) and is only claimed statistically against the reference.
//  * k_mmd<M>: maximum mean discrepancy between two particle sets (AMP `mmd`), one 256-thread block per pair of sets.
//  * k_kde_eval<M>: log-density of a belief's kernel density estimate at query points (the belief called as a function, AMP
//    `evaluateDualTree`), one 256-thread block per (belief, tile of 256 queries).
// All are written once over a manifold policy M (Flat<2> Point2, Flat<3> Pose2, Se3M Pose3), which holds everything that
// differs between the variable types.  Belief statistics: one wave (64-thread block) per variable.  Product: one 256-thread
// block per variable (see k_product); weights are scanned in particle order so the resampling picks are the same as a
// sequential CPU scan.
#include <cmath>

#include "rome_device_math.hpp"
#include "rome_kernels.h"

namespace rome {

constexpr int kProdMaxN = 512;

// ---- manifold policies -----------------------------------------------------------------------------------------------------
// Pt: a point in registers, kLds doubles of it per LDS slot (put / get), staged(S): whether the product stages the points of a
// proposal in LDS.  diff: tangent coordinates of x about y.  dist2: Σ (diff_k · ih_k)², summed in the order of the oracle.
// retract: x moved by e in its own chart, as coordinates.  jitter: retract as the product stores it.

// flat coordinates: Point2 (D = 2), Pose2 (D = 3: coordinate 2 is a heading, differences wrapped)
template <int D_>
struct Flat {
  static constexpr int D = D_, kLds = D_;
  static constexpr bool staged(int S) { return S <= 4; }   // N <= 256; beyond, points come through wave-uniform global loads
  struct Pt { double c[D]; };
  static __device__ __forceinline__ void load(const double* __restrict__ P, int N, int i, Pt& a) {
#pragma unroll
    for (int k = 0; k < D; ++k) a.c[k] = P[k * N + i];
  }
  static __device__ __forceinline__ void diff(const Pt& x, const Pt& y, double (&d)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) { const double e = x.c[k] - y.c[k]; d[k] = (D == 3 && k == 2) ? wrap_pi(e) : e; }
  }
  static __device__ __forceinline__ double dist2(const Pt& x, const Pt& y, const double (&ih)[D]) {
    double d[D], q = 0.0;
    diff(x, y, d);
#pragma unroll
    for (int k = 0; k < D; ++k) { const double s = d[k] * ih[k]; q += s * s; }
    return q;
  }
  template <class A> static __device__ __forceinline__ void put(A& lds, int i, const Pt& a) {
#pragma unroll
    for (int k = 0; k < D; ++k) lds[k][i] = a.c[k];
  }
  template <class A> static __device__ __forceinline__ void get(const A& lds, int j, Pt& a) {
#pragma unroll
    for (int k = 0; k < D; ++k) a.c[k] = lds[k][j];
  }
  static __device__ __forceinline__ void retract(const Pt& x, const double (&e)[D], double (&o)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) o[k] = x.c[k] + e[k];
  }
  static __device__ __forceinline__ void jitter(const Pt& x, const double (&e)[D], double (&o)[D]) {
    retract(x, e, o);
    if constexpr (D == 3) o[2] = wrap_pi(o[2]);   // product outputs only: the stats mean heading stays θ₀ + mean d, as the oracle's
  }
};

// SE(3), coordinates [t(3); rotation vector(3)]:  d(x, y) = (x.t − y.t, Log(R_yᵀ R_x)),  x ⊕ e = (t + e_t, R Exp(e_ω)).
// Rotations are unit quaternions from load to store: one Exp per point when it is loaded or staged, one Log per pair.  A matrix
// logarithm through acos(c) and sqrt(1 − c²) loses 1e-16 / sin²θ of the angle, 1e-10 rad at π − 1e-3.
struct Se3M {
  static constexpr int D = 6, kLds = 7;
  static constexpr bool staged(int) { return true; }       // (t, q) of every point of a proposal: N <= 256
  struct Pt { double t[3], q[4]; };
  static __device__ __forceinline__ void load(const double* __restrict__ P, int N, int i, Pt& a) {
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.t[k] = P[k * N + i]; w[k] = P[(3 + k) * N + i]; }
    quat_exp(w, a.q);
  }
  static __device__ __forceinline__ void diff(const Pt& x, const Pt& y, double (&d)[6]) {
    double e[4];
    quat_cmul(y.q, x.q, e);
    quat_log(e, d + 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = x.t[k] - y.t[k];
  }
  static __device__ __forceinline__ double dist2(const Pt& x, const Pt& y, const double (&ih)[6]) {
    double d[6], q = 0.0;
    diff(x, y, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double dt = d[k] * ih[k]; q += dt * dt; const double dw = d[3 + k] * ih[3 + k]; q += dw * dw; }
    return q;
  }
  template <class A> static __device__ __forceinline__ void put(A& lds, int i, const Pt& a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) lds[k][i] = a.t[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) lds[3 + k][i] = a.q[k];
  }
  template <class A> static __device__ __forceinline__ void get(const A& lds, int j, Pt& a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.t[k] = lds[k][j];
#pragma unroll
    for (int k = 0; k < 4; ++k) a.q[k] = lds[3 + k][j];
  }
  static __device__ __forceinline__ void retract(const Pt& x, const double (&e)[6], double (&o)[6]) {
    double qe[4], qn[4];
    quat_exp(e + 3, qe); quat_mul(x.q, qe, qn); quat_log(qn, o + 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = x.t[k] + e[k];
  }
  static __device__ __forceinline__ void jitter(const Pt& x, const double (&e)[6], double (&o)[6]) { retract(x, e, o); }
};
template <int D> struct ManifoldOf { using type = Flat<D>; };
template <> struct ManifoldOf<6> { using type = Se3M; };

// per-coordinate (mean offset, std) of the tangent coordinates about particle 0 of one SoA block; all lanes get the result
template <class M>
__device__ __forceinline__ void block_stats(const double* __restrict__ P, int N, double inv_n, double inv_nm1, int lane,
                                            typename M::Pt& x0, double (&moff)[M::D], double (&sd)[M::D]) {
  constexpr int D = M::D;
  M::load(P, N, 0, x0);
  double s[2 * D];
#pragma unroll
  for (int j = 0; j < 2 * D; ++j) s[j] = 0.0;
  for (int i = lane; i < N; i += 64) {
    typename M::Pt xi; M::load(P, N, i, xi);
    double d[D]; M::diff(xi, x0, d);
#pragma unroll
    for (int k = 0; k < D; ++k) { s[2 * k] += d[k]; s[2 * k + 1] += d[k] * d[k]; }
  }
  wave_sum_n<2 * D>(s);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    moff[k] = s[2 * k] * inv_n;
    sd[k] = fast_sqrt(fmax(0.0, (s[2 * k + 1] - s[2 * k] * s[2 * k] * inv_n) * inv_nm1));
  }
}

template <int D>
__global__ void __launch_bounds__(64) k_belief_stats(int V, int N, double inv_n, double inv_nm1, const double* __restrict__ bel,
                                                     double* __restrict__ mean, double* __restrict__ sdev) {
  using M = typename ManifoldOf<D>::type;
  const int v = blockIdx.x;
  if (v >= V) return;
  const int lane = threadIdx.x;
  typename M::Pt x0;
  double moff[D], sd[D], m[D];
  block_stats<M>(bel + (size_t)v * D * N, N, inv_n, inv_nm1, lane, x0, moff, sd);
  M::retract(x0, moff, m);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) { mean[D * v + k] = m[k]; sdev[D * v + k] = sd[k]; }
  }
}

// ---- mmd: maximum mean discrepancy between two particle sets ------------------------------------------------------------------
// out[p] = S_aa/Na² − 2 S_ab/(Na Nb) + S_bb/Nb² with S_xy = Σ_{i,j} exp(−σ · M::dist2(x_i, y_j, scale)) over all ordered pairs (the
// biased V-statistic of MMD², as AMP's `mmd`).  One 256-thread block per pair p of blocks (a_rows[p], b_rows[p]).  Both sets are
// staged once in dynamic LDS ((Na + Nb) · M::kLds doubles) by M::load / M::put: one quat_exp per point, none per pair.  Each panel's
// pair index is flattened over the threads (at N = 100 a row per thread would idle 61 % of the block); the aa and bb panels visit
// every UNORDERED pair i != j once -- in circulant order (r, (r + c) mod n), so both i < j and i > j occur: dist2 is symmetric --, are
// doubled and get their exact diagonal Na / Nb.  Three per-thread sums, wave_sum_n<3>, then the four waves in
// a fixed order: no atomics, so the bits of out[p] depend on pair p's inputs alone.
constexpr int kMmdThreads = 256;
constexpr int kMmdMaxN = 512;

struct MmdArgs {
  int Na, Nb;
  const double* a;         // [rows][D][Na]
  const int32_t* a_rows;   // [P] block of `a` of pair p, or null: p
  const double* b;         // [rows][D][Nb]
  const int32_t* b_rows;
  double scale[6];         // per-coordinate weights s_c >= 0 (0 drops the coordinate)
  double sigma;
  double* out;             // [P]
  double* sums;            // [P][3] = S_aa, S_ab, S_bb, or null
};

// [M::kLds][n] lines in dynamic LDS, indexed as M::put / M::get index their array
struct LdsLines {
  double* p; int n;
  __device__ __forceinline__ double* operator[](int k) const { return p + k * n; }
};

// (t / n, t % n) of the flattened indices t = tid, tid + 256, ... one thread visits: one division, then additions
struct PairWalk {
  int q, r, dq, dr, n;
  __device__ __forceinline__ PairWalk(int tid, int n_) : q(tid / n_), r(tid % n_), dq(kMmdThreads / n_), dr(kMmdThreads % n_), n(n_) {}
  __device__ __forceinline__ void next() { q += dq; r += dr; if (r >= n) { r -= n; ++q; } }
};

template <class M>
__device__ __forceinline__ void mmd_stage(const double* __restrict__ P, int N, int tid, const LdsLines& X) {
  for (int i = tid; i < N; i += kMmdThreads) { typename M::Pt x; M::load(P, N, i, x); M::put(X, i, x); }
}
// Σ over the unordered pairs i != j of one set.  Pair t = (c − 1)·n + r is (r, (r + c) mod n), c = 1 .. n/2: every unordered pair
// once (n even: the last c only for r < n/2, which is where t < n(n−1)/2 ends).
template <class M>
__device__ __forceinline__ double mmd_triangle(const LdsLines& X, int n, int tid, const double (&w)[M::D], double neg_sigma) {
  double acc = 0.0;
  const int T = n * (n - 1) / 2;
  PairWalk pw(tid, n);
  for (int t = tid; t < T; t += kMmdThreads, pw.next()) {
    const int i = pw.r;
    int j = i + pw.q + 1;
    if (j >= n) j -= n;
    typename M::Pt x, y;
    M::get(X, i, x); M::get(X, j, y);
    acc += fast_exp_neg(neg_sigma * M::dist2(x, y, w));
  }
  return acc;
}
// Σ over the full rectangle (i, j) = (t / nb, t % nb)
template <class M>
__device__ __forceinline__ double mmd_rectangle(const LdsLines& A, int na, const LdsLines& B, int nb, int tid, const double (&w)[M::D],
                                                double neg_sigma) {
  double acc = 0.0;
  const int T = na * nb;
  PairWalk pw(tid, nb);
  for (int t = tid; t < T; t += kMmdThreads, pw.next()) {
    typename M::Pt x, y;
    M::get(A, pw.q, x); M::get(B, pw.r, y);
    acc += fast_exp_neg(neg_sigma * M::dist2(x, y, w));
  }
  return acc;
}

template <class M>
__global__ void __launch_bounds__(kMmdThreads) k_mmd(const MmdArgs g) {
  constexpr int D = M::D;
  extern __shared__ double mmd_pts[];
  __shared__ double red[kMmdThreads / 64][3];
  const int p = blockIdx.x, tid = threadIdx.x, Na = g.Na, Nb = g.Nb;
  const LdsLines A{mmd_pts, Na}, B{mmd_pts + M::kLds * Na, Nb};
  mmd_stage<M>(g.a + (size_t)(g.a_rows ? g.a_rows[p] : p) * D * Na, Na, tid, A);
  mmd_stage<M>(g.b + (size_t)(g.b_rows ? g.b_rows[p] : p) * D * Nb, Nb, tid, B);
  __syncthreads();
  double w[D];
#pragma unroll
  for (int k = 0; k < D; ++k) w[k] = g.scale[k];
  const double ns = -g.sigma;
  double acc[3];
  acc[0] = mmd_triangle<M>(A, Na, tid, w, ns);
  acc[1] = mmd_rectangle<M>(A, Na, B, Nb, tid, w, ns);
  acc[2] = mmd_triangle<M>(B, Nb, tid, w, ns);
  wave_sum_n<3>(acc);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) red[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid == 0) {
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    const double saa = 2.0 * s[0] + (double)Na, sab = s[1], sbb = 2.0 * s[2] + (double)Nb;
    // IEEE divisions (one thread, once): a sum that is exactly its pair count gives exactly 1
    const double taa = saa / ((double)Na * (double)Na), tab = sab / ((double)Na * (double)Nb), tbb = sbb / ((double)Nb * (double)Nb);
    g.out[p] = (taa - tab) + (tbb - tab);
    if (g.sums) { g.sums[3 * p] = saa; g.sums[3 * p + 1] = sab; g.sums[3 * p + 2] = sbb; }
  }
}

// ---- kde_eval: log-density of a belief at query points -------------------------------------------------------------------------
// out[p][i] = −½ q_min + log Σ_j exp(−½ (q_j − q_min)) − log N' − Σ_k log h_k − (D/2) log 2π,  q_j = M::dist2(x_i, y_j, 1/h) (saturated
// at 1e300, so that the result is finite for every finite input), j in particle order, the running-minimum sum of k_product.  Block
// b serves pair p = b / tiles and queries 256·(b mod tiles) ..: the N points of belief block bel_rows[p] are staged once in dynamic LDS
// (M::load / M::put: one quat_exp per point), then each thread owns one query and walks the points at a wave-uniform LDS address.
// The arithmetic of a query is that of its thread alone and does not involve tid: the bits of out[p][i] depend on the belief block, its
// bandwidth row and the query, not on Q, P or the query's place.  Self-evaluation (queries == null, Q == N) loads the queries from the
// belief block through the same M::load; leave-one-out skips j == i and counts N' = N − 1.
constexpr int kKdeEvalThreads = 256;
constexpr int kKdeEvalMaxN = 512;

struct KdeEvalArgs {
  int N, Q, tiles, loo;
  const double* bel;           // [rows][D][N]
  const int32_t* bel_rows;     // [P] block of `bel` (and row of `bw`) of pair p, or null: p
  const double* bw;            // [rows][D]
  const double* queries;       // [rows][D][Q], or null: the pair's own belief block (Q == N)
  const int32_t* query_rows;
  double c0;                   // log N' + (D/2) log 2π
  double* out;                 // [P][Q]
};

template <class M>
__global__ void __launch_bounds__(kKdeEvalThreads) k_kde_eval(const KdeEvalArgs g) {
  constexpr int D = M::D;
  extern __shared__ double kde_eval_pts[];
  const int tid = threadIdx.x, N = g.N, Q = g.Q;
  const int p = blockIdx.x / g.tiles, tile = blockIdx.x - p * g.tiles;
  const int brow = g.bel_rows ? g.bel_rows[p] : p;
  const double* B = g.bel + (size_t)brow * D * N;
  const LdsLines Y{kde_eval_pts, N};
  mmd_stage<M>(B, N, tid, Y);
  __syncthreads();
  const int i = tile * kKdeEvalThreads + tid;
  if (i >= Q) return;
  const double* X = g.queries ? g.queries + (size_t)(g.query_rows ? g.query_rows[p] : p) * D * Q : B;
  typename M::Pt x;
  M::load(X, Q, i, x);
  double ih[D], lnh = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) { const double h = g.bw[(size_t)brow * D + k]; ih[k] = 1.0 / h; lnh += fast_log(h); }
  const int skip = g.loo ? i : -1;
  double qmin = __builtin_inf(), sacc = 0.0;
  for (int j = 0; j < N; ++j) {
    if (j == skip) continue;
    typename M::Pt y;
    M::get(Y, j, y);
    const double q = fmin(M::dist2(x, y, ih), 1e300);
    const double dq = q - qmin;
    const double e = fast_exp_neg(-0.5 * fabs(dq));
    sacc = dq < 0.0 ? fma(sacc, e, 1.0) : sacc + e;
    qmin = fmin(qmin, q);
  }
  g.out[(size_t)p * Q + i] = ((-0.5 * qmin + fast_log(sacc)) - lnh) - g.c0;
}

struct ProductArgs {
  int V, N;
  const int32_t* prop_ptr;   // [V+1]
  const int32_t* prop_rows;  // rows of `prop` targeting each variable
  const double* prop;        // [rows][D][N]
  const double* prop_bw;     // [rows][D] kernel bandwidths of the proposals (rome_kde_bandwidth_dev), or null: Silverman in-kernel
  const double* bel_in;      // [V][D][N]
  double* bel_out;           // [V][D][N]
  double inv_n, inv_nm1, c_n;  // c_n: Silverman factor (4/((d+2)N))^(1/(d+4)), host-computed
  uint64_t seed, stream_offset;
};

// One 256-thread block (4 wavefronts) per variable.  The K-1 non-base proposals are dealt round-robin to the four
// waves -- a variable with many proposals (loop-closure hubs: K up to ~11 on Manhattan) no longer serialises them in
// one wave.  Inside a wave, lane l owns base particles l, l+64, ... (S slots, N <= 64·S) and walks the N kernel points
// of its proposal at a wave-uniform address (its own LDS region where M stages them, scalar-cache loads otherwise); the
// per-proposal log-weight contributions go to LDS and are summed per particle in proposal order, so the arithmetic order
// -- and the resampling picks -- are those of the sequential definition in oracle/rome_oracle.c (ro_product).
constexpr int kProdWaves = 4;
constexpr int kProdChunk = 8;   // proposals whose contributions are buffered in LDS at a time
constexpr int kProdMaxK = 32;   // proposals whose bandwidths are kept in LDS (more: recomputed where needed)

// kernel bandwidths of one proposal: caller-supplied (leave-one-out likelihood rule, rome_kde.hip) or Silverman's rule on
// the proposal's spread; floored at 1e-6 either way
template <class M>
__device__ __forceinline__ void proposal_bandwidth(const ProductArgs& a, int row, const double* __restrict__ P, int N, int lane,
                                                   double (&h)[M::D]) {
  constexpr int D = M::D;
  if (a.prop_bw) {
#pragma unroll
    for (int k = 0; k < D; ++k) h[k] = fmax(a.prop_bw[(size_t)row * D + k], 1e-6);   // wave-uniform address
  } else {
    typename M::Pt x0;
    double moff[D], sd[D];
    block_stats<M>(P, N, a.inv_n, a.inv_nm1, lane, x0, moff, sd);
#pragma unroll
    for (int k = 0; k < D; ++k) h[k] = fmax(a.c_n * sd[k], 1e-6);
  }
}

#ifndef ROME_PROD3_MINBLK
#define ROME_PROD3_MINBLK 3   // blocks per CU: 3 waves/SIMD (168 VGPRs, a few spills) measured 1.67 ms vs 2.10 (2) and 2.49 (4) on the 10^4-pose helix
#endif
template <class M, int S>
__global__ void __launch_bounds__(64 * kProdWaves, M::D == 6 ? ROME_PROD3_MINBLK : 1) k_product(const ProductArgs a) {
  constexpr int D = M::D;
  using Pt = typename M::Pt;
  constexpr int T4 = (S + kProdWaves - 1) / kProdWaves;   // particles per thread in the block-wide phases
  constexpr bool kStage = M::staged(S);   // every wave stages the points of its proposal in its own LDS region
  __shared__ double pts[kStage ? kProdWaves : 1][M::kLds][kStage ? 64 * S : 1];
  __shared__ double contrib[kProdChunk][64 * S];
  __shared__ double wts[64 * S];
  __shared__ double red[kProdWaves];
  __shared__ double ihbuf[kProdMaxK][D];
  __shared__ double lnbuf[kProdMaxK];
  const int v = blockIdx.x;
  if (v >= a.V) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), N = a.N;
  const int r0 = a.prop_ptr[v], K = a.prop_ptr[v + 1] - r0;
  double* ob = a.bel_out + (size_t)v * D * N;
  if (K <= 1) {
    const double* src = K == 0 ? a.bel_in + (size_t)v * D * N : a.prop + (size_t)a.prop_rows[r0] * D * N;
    for (int i = tid; i < D * N; i += 64 * kProdWaves) ob[i] = src[i];
    return;
  }
  // pass 1: bandwidths (proposals dealt to the waves, exchanged through LDS), base proposal, product bandwidth
  int base = 0;
  double best = __builtin_inf();
  double hp_acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) hp_acc[k] = 0.0;
  for (int l0 = 0; l0 < K; l0 += kProdMaxK) {
    const int cnt = min(kProdMaxK, K - l0);
    for (int c = wave; c < cnt; c += kProdWaves) {
      const int row = a.prop_rows[r0 + l0 + c];
      double h[D];
      proposal_bandwidth<M>(a, row, a.prop + (size_t)row * D * N, N, lane, h);
      double ln = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        ln += fast_log(h[k]);
        if (lane == 0) ihbuf[c][k] = 1.0 / h[k];
      }
      if (lane == 0) lnbuf[c] = ln;
    }
    __syncthreads();
    for (int c = 0; c < cnt; ++c) {
#pragma unroll
      for (int k = 0; k < D; ++k) { const double ih = ihbuf[c][k]; hp_acc[k] = fma(ih, ih, hp_acc[k]); }
      const double ln = lnbuf[c];
      if (ln < best) { best = ln; base = l0 + c; }
    }
    if (l0 + kProdMaxK < K) __syncthreads();   // the buffers are reused by the next chunk
  }
  const bool h_cached = K <= kProdMaxK;        // single chunk: ihbuf still holds every proposal's 1/h
  const double* __restrict__ Pb = a.prop + (size_t)a.prop_rows[r0 + base] * D * N;
  // pass 2: log weights of the base particles
  Pt x[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { const int i = lane + 64 * s; M::load(Pb, N, i < N ? i : 0, x[s]); }
  double lw[T4];
#pragma unroll
  for (int s = 0; s < T4; ++s) lw[s] = 0.0;
  for (int c0 = 0; c0 < K - 1; c0 += kProdChunk) {          // chunk of non-base proposals c0 .. c0+cnt-1
    const int cnt = min(kProdChunk, K - 1 - c0);
    for (int c = wave; c < cnt; c += kProdWaves) {
      const int nb = c0 + c, l = nb < base ? nb : nb + 1;   // nb-th non-base proposal
      const int row = a.prop_rows[r0 + l];
      const double* __restrict__ P = a.prop + (size_t)row * D * N;
      double ih[D];
      if (h_cached) {
#pragma unroll
        for (int k = 0; k < D; ++k) ih[k] = ihbuf[l][k];
      } else {
        double h[D];
        proposal_bandwidth<M>(a, row, P, N, lane, h);
#pragma unroll
        for (int k = 0; k < D; ++k) ih[k] = 1.0 / h[k];
      }
      double qmin[S], sacc[S];
#pragma unroll
      for (int s = 0; s < S; ++s) { qmin[s] = __builtin_inf(); sacc[s] = 0.0; }
      // one pass, running log-sum-exp: sacc = Σ_j exp(-½(q_j - qmin)) with qmin the smallest q seen so far
      if constexpr (kStage) {   // wave-private LDS region: only wave-level ordering is needed
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int i = lane + 64 * s;
          if (i < N) { Pt y; M::load(P, N, i, y); M::put(pts[wave], i, y); }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      }
      for (int j = 0; j < N; ++j) {
        Pt y;
        if constexpr (kStage) M::get(pts[wave], j, y); else M::load(P, N, j, y);   // wave-uniform address
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if (lane + 64 * s < N) {  // skip idle slots (keeps exp() off them)
            const double q = M::dist2(x[s], y, ih);
            const double dq = q - qmin[s];
            const double e = fast_exp_neg(-0.5 * fabs(dq));
            sacc[s] = dq < 0.0 ? fma(sacc[s], e, 1.0) : sacc[s] + e;
            qmin[s] = fmin(qmin[s], q);
          }
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) if (lane + 64 * s < N) contrib[c][lane + 64 * s] = -0.5 * qmin[s] + fast_log(sacc[s]);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < T4; ++s) {
      const int i = tid + 64 * kProdWaves * s;
      if (i < N) for (int c = 0; c < cnt; ++c) lw[s] += contrib[c][i];   // proposal order
    }
    __syncthreads();
  }
  // normalise, publish weights in particle order
  double mx = -__builtin_inf();
#pragma unroll
  for (int s = 0; s < T4; ++s) if (tid + 64 * kProdWaves * s < N) mx = fmax(mx, lw[s]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
#pragma unroll
  for (int s = 0; s < T4; ++s) { const int i = tid + 64 * kProdWaves * s; if (i < N) wts[i] = exp(lw[s] - mx); }
  __syncthreads();
  // systematic resampling: cumulative weights by a sequential scan in particle order (one wave; same arithmetic
  // order as a CPU loop), then every thread looks its picks up by bisection (first m with cum[m] > τ, else N-1)
  if (wave == 0) {
    double cum = 0.0;
    for (int m = 0; m < N; ++m) {
      cum += wts[m];
      if (lane == (m & 63)) contrib[0][m] = cum;   // contrib is free again: reuse its first row
    }
  }
  __syncthreads();
  const double* cumw = contrib[0];
  const double T = cumw[N - 1];
  const uint64_t stream = a.stream_offset + (uint64_t)v;
  const u32x4 uw = philox4x32_10(u32x4{0xFFFFFFFFu, (uint32_t)stream, (uint32_t)(stream >> 32), (3u << 16)},
                                 (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  const double u = ((double)uw.x + 0.5) * (1.0 / 4294967296.0);
  int pick[T4];
#pragma unroll
  for (int s = 0; s < T4; ++s) {
    const int i = tid + 64 * kProdWaves * s;
    if (i < N) {
      const double tau = ((double)i + u) * T / (double)N;
      int lo = 0, hi = N - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cumw[mid] > tau) hi = mid; else lo = mid + 1;
      }
      pick[s] = lo;
    }
  }
#pragma unroll
  for (int s = 0; s < T4; ++s) {
    const int i = tid + 64 * kProdWaves * s;
    if (i < N) {
      Pt p; M::load(Pb, N, pick[s], p);
      double xi[D], e[D], o[D];
      rng_normals<D>(a.seed, stream, (uint32_t)i, xi);
#pragma unroll
      for (int k = 0; k < D; ++k) e[k] = xi[k] / fast_sqrt(hp_acc[k]);
      M::jitter(p, e, o);
#pragma unroll
      for (int k = 0; k < D; ++k) ob[k * N + i] = o[k];
    }
  }
}

hipError_t launch_belief_stats(int dim, int V, int N, const double* bel, double* mean, double* sdev, hipStream_t s) {
  if (V <= 0) return hipSuccess;
  const double inv_n = 1.0 / N, inv_nm1 = N > 1 ? 1.0 / (N - 1) : 1.0;
  switch (dim) {
    case 2: hipLaunchKernelGGL(k_belief_stats<2>, dim3(V), dim3(64), 0, s, V, N, inv_n, inv_nm1, bel, mean, sdev); break;
    case 3: hipLaunchKernelGGL(k_belief_stats<3>, dim3(V), dim3(64), 0, s, V, N, inv_n, inv_nm1, bel, mean, sdev); break;
    case 6: hipLaunchKernelGGL(k_belief_stats<6>, dim3(V), dim3(64), 0, s, V, N, inv_n, inv_nm1, bel, mean, sdev); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <class M>
static hipError_t launch_mmd_of(int P, const MmdArgs& g, hipStream_t s) {
  const size_t lds = sizeof(double) * M::kLds * ((size_t)g.Na + (size_t)g.Nb);   // <= 56 KiB at 512 + 512 Pose3 points
  hipLaunchKernelGGL(k_mmd<M>, dim3(P), dim3(kMmdThreads), lds, s, g);
  return hipGetLastError();
}

hipError_t launch_mmd(int dim, int P, int Na, const double* a, const int32_t* a_rows, int Nb, const double* b, const int32_t* b_rows,
                      const double* scale, double sigma, double* out, double* sums, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  if (Na < 1 || Nb < 1 || Na > kMmdMaxN || Nb > kMmdMaxN) return hipErrorInvalidValue;
  MmdArgs g;
  g.Na = Na; g.Nb = Nb; g.a = a; g.a_rows = a_rows; g.b = b; g.b_rows = b_rows; g.sigma = sigma; g.out = out; g.sums = sums;
  for (int k = 0; k < 6; ++k) g.scale[k] = (scale && k < dim) ? scale[k] : 1.0;
  if (dim == 2) return launch_mmd_of<Flat<2>>(P, g, s);
  if (dim == 3) return launch_mmd_of<Flat<3>>(P, g, s);
  if (dim == 6) return launch_mmd_of<Se3M>(P, g, s);
  return hipErrorInvalidValue;
}

template <class M>
static hipError_t launch_kde_eval_of(int P, const KdeEvalArgs& g, hipStream_t s) {
  const size_t lds = sizeof(double) * M::kLds * (size_t)g.N;   // <= 28 KiB at 512 Pose3 points
  hipLaunchKernelGGL(k_kde_eval<M>, dim3((unsigned)(P * g.tiles)), dim3(kKdeEvalThreads), lds, s, g);
  return hipGetLastError();
}

hipError_t launch_kde_eval(int dim, int P, int N, const double* bel, const int32_t* bel_rows, const double* bw, int Q, const double* queries,
                           const int32_t* query_rows, int leave_one_out, double* out, hipStream_t s) {
  if (P <= 0 || Q <= 0) return hipSuccess;
  if (N < 1 || N > kKdeEvalMaxN || (!queries && Q != N) || (leave_one_out && (queries || N < 2))) return hipErrorInvalidValue;
  KdeEvalArgs g;
  g.N = N; g.Q = Q; g.tiles = (Q - 1) / kKdeEvalThreads + 1; g.loo = leave_one_out ? 1 : 0;
  if ((long long)P * g.tiles > 0x7fffffffLL) return hipErrorInvalidValue;   // blocks of a 1-D grid
  g.bel = bel; g.bel_rows = bel_rows; g.bw = bw; g.queries = queries; g.query_rows = query_rows; g.out = out;
  g.c0 = std::log((double)(leave_one_out ? N - 1 : N)) + 0.5 * dim * 1.8378770664093453;   // log 2π
  if (dim == 2) return launch_kde_eval_of<Flat<2>>(P, g, s);
  if (dim == 3) return launch_kde_eval_of<Flat<3>>(P, g, s);
  if (dim == 6) return launch_kde_eval_of<Se3M>(P, g, s);
  return hipErrorInvalidValue;
}

// S slots per lane from N.  A manifold that stages at every S has no S = 8 kernel (its points would not fit in LDS): N <= 256.
template <class M>
static hipError_t launch_product_of(const ProductArgs& a, hipStream_t s) {
  const dim3 grid(a.V), block(64 * kProdWaves);
  if (a.N <= 64) hipLaunchKernelGGL((k_product<M, 1>), grid, block, 0, s, a);
  else if (a.N <= 128) hipLaunchKernelGGL((k_product<M, 2>), grid, block, 0, s, a);
  else if (a.N <= 256) hipLaunchKernelGGL((k_product<M, 4>), grid, block, 0, s, a);
  else if constexpr (M::staged(8)) return hipErrorInvalidValue;
  else hipLaunchKernelGGL((k_product<M, 8>), grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_product(int dim, int V, int N, const int32_t* prop_ptr, const int32_t* prop_rows, const double* prop,
                          const double* prop_bw, const double* bel_in, double* bel_out, double c_n, uint64_t seed,
                          uint64_t stream_offset, hipStream_t s) {
  if (V <= 0) return hipSuccess;
  if (N > kProdMaxN) return hipErrorInvalidValue;
  ProductArgs a;
  a.V = V; a.N = N; a.prop_ptr = prop_ptr; a.prop_rows = prop_rows; a.prop = prop; a.prop_bw = prop_bw; a.bel_in = bel_in; a.bel_out = bel_out;
  a.inv_n = 1.0 / N; a.inv_nm1 = N > 1 ? 1.0 / (N - 1) : 1.0; a.c_n = c_n; a.seed = seed; a.stream_offset = stream_offset;
  if (dim == 2) return launch_product_of<Flat<2>>(a, s);
  if (dim == 3) return launch_product_of<Flat<3>>(a, s);
  if (dim == 6) return launch_product_of<Se3M>(a, s);
  return hipErrorInvalidValue;
}

}  // namespace rome
