// rome_upsolve_index.h -- everything about the clique entries and an up-solve plan that is not a HIP call: the five row families of a
// rome_clique_host, the update index of a rome_clique_upsolve_host (what a plan's launches are derived from), and the layout of the three
// device arenas of rome_capi_clique.hip, each written ONCE as a function of an arena cursor: run with a measuring cursor it gives the
// arena's size, run again with a placing cursor over an allocation of that size it gives the pointers and the copies owed.  No HIP: a
// host-only program compiles it (tests/c/upsolve_index_check.cpp).
#pragma once
#include "../../include/rome_mi355.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rome {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
constexpr int kVdim[3] = {3, 2, 6};   // variable types: 0 Pose2, 1 Point2, 2 Pose3

// the five row families of a rome_clique_host.  kind: 0 Pose2Pose2 (+ PriorPose2 rows), 1 bearing-range, 2 Pose3Pose3 (+ PriorPose3 rows),
// 3 PriorPoint2 sampler; valt = type of the array an `alt` entry indexes (-1: no multihypo); base = first row of the family in the
// proposal buffer of its target type (up-solve plans)
struct Fam {
  int n; const int32_t* rows4; int F; const double* mu; const double* spread; int dz, nL, dfx, dt; double* out; int vf, vt; int dir_all;
  uint64_t off; int kind; int base;
  const int32_t* alt; const double* hw; const double* nh; const int32_t* sid; int valt;
  const int32_t* meas;   // per-row block of the measurement samples (Pose2Pose2 / bearing-range / Pose3Pose3 rows), or nullptr
  int vmeas() const { return kind == 1 ? 1 : (kind == 2 ? 2 : 0); }   // variable type of the store array a `meas` entry indexes
};
constexpr int NF = 5;
inline void make_fams(const rome_clique_host* q, Fam (&fam)[NF]) {
  const Fam f[NF] = {
    {q->n_p2p2, q->p2p2_rows4, q->f_p2p2, q->p2p2_mu, q->p2p2_cov, 3, 6, 3, 3, q->out_p2p2, 0, 0, 0, 0ull, 0, 0,
     q->p2p2_alt, q->p2p2_hypo_w, q->p2p2_nullhypo, q->p2p2_stream, 0, q->p2p2_meas},
    {q->n_br1, q->br1_rows4, q->f_br, q->br_mu, q->br_sigma, 2, 2, 2, 3, q->out_br1, 1, 0, 1, 1ull << 28, 1, q->n_p2p2,
     q->br1_alt, q->br1_hypo_w, q->br1_nullhypo, q->br1_stream, 1, q->br1_meas},
    {q->n_br0, q->br0_rows4, q->f_br, q->br_mu, q->br_sigma, 2, 2, 3, 2, q->out_br0, 0, 1, 0, 2ull << 28, 1, 0,
     q->br0_alt, q->br0_hypo_w, q->br0_nullhypo, q->br0_stream, 1, q->br0_meas},
    {q->n_p3p3, q->p3p3_rows4, q->f_p3p3, q->p3p3_mu, q->p3p3_cov, 6, 21, 6, 6, q->out_p3p3, 2, 2, 0, 5ull << 28, 2, 0,
     nullptr, nullptr, q->p3p3_nullhypo, q->p3p3_stream, -1, q->p3p3_meas},
    {q->n_prpt2, q->prpt2_rows4, q->f_prpt2, q->prpt2_mu, q->prpt2_cov, 2, 3, 2, 2, q->out_prpt2, 1, 1, 0, 7ull << 28, 3, q->n_br0,
     nullptr, nullptr, nullptr, q->prpt2_stream, -1, nullptr}};
  for (int k = 0; k < NF; ++k) fam[k] = f[k];
}
// table entries must address the arrays they index (nv = variables per type); hypothesis / stream columns in range
inline int check_fam_rows(const Fam& f, const int (&nv)[3]) {
  if (f.n < 0 || f.F < 0 || (f.n > 0 && (!f.rows4 || !f.mu || !f.spread || f.F == 0))) return ROME_ERR_INVALID_ARG;
  if (f.alt && !f.hw) return ROME_ERR_INVALID_ARG;
  for (int r = 0; r < f.n; ++r) {
    const int32_t* e = f.rows4 + 4 * (size_t)r;
    if (e[0] < 0 || e[0] >= f.F || e[2] < 0 || e[2] >= nv[f.vf] || e[3] < 0 || e[3] >= nv[f.vt] || e[1] < 0 || e[1] > 2) return ROME_ERR_INVALID_ARG;
    if (f.alt && f.alt[r] >= 0) {
      if (f.alt[r] >= nv[f.valt] || !(f.hw[r] >= 0.0 && f.hw[r] <= 1.0)) return ROME_ERR_INVALID_ARG;
    } else if (f.alt && f.alt[r] < -1) return ROME_ERR_INVALID_ARG;
    if (f.nh && !(f.nh[r] >= 0.0 && f.nh[r] <= 1.0)) return ROME_ERR_INVALID_ARG;
    if (f.sid && (f.sid[r] < 0 || f.sid[r] >= (1 << 28))) return ROME_ERR_INVALID_ARG;
    if (f.meas && (f.meas[r] < -1 || f.meas[r] >= nv[f.vmeas()] || (f.meas[r] >= 0 && e[1] == 2))) return ROME_ERR_INVALID_ARG;
  }
  return ROME_OK;
}

/* ---- the update index of a rome_clique_upsolve_host ---- */
// one variable type: its n_up updated variables and the prop_rows rows of its proposal buffer -- the family rows (from Fam::base), then
// n_msg host messages from msg_base, then n_smsg store-resident messages from smsg_base
struct TypeCounts {
  int n_up = 0, n_msg = 0, msg_base = 0, n_smsg = 0, smsg_base = 0, prop_rows = 0;
  int max_k = 1;   // most proposals of one product
};
struct TypeIndex : TypeCounts {   // ... and the type's tables, as they are uploaded
  std::vector<int> up;                          // positions in the update list of the type's updated variables, in update order
  std::vector<int32_t> ptr, rows;               // CSR over them: the rows of the type's proposal buffer that enter each variable's product
  std::vector<int32_t> block, stream, mirror;   // per updated variable: its store block, Philox stream id, mirror block (-1: none)
  std::vector<int32_t> gather;                  // (dim, var, position, type) per updated variable: store -> contiguous download buffer
  std::vector<int32_t> smsg;                    // (dim, source block, proposal row, type) per store-resident message
};
struct UpsolveSteps {   // what the launches of a run are derived from (a plan keeps this part)
  int n_up = 0;
  bool has_mirror = false, has_upstream = false;
  Fam fam[NF];
  std::vector<int> fam_lo[NF];      // first row of family f that targets update position >= k (rows are grouped in update order)
  std::vector<int> step_k;          // boundaries of the update steps (ranges of the update list updated together)
  std::vector<int> up_cnt_before;   // [k][t]: updates of type t among the first k
};
struct UpsolveIndex : UpsolveSteps { TypeIndex type[3]; };

// validates `u` over a store of nv[t] variables per type and fills X -> ROME_OK or the code an up-solve entry returns for this table
inline int index_upsolve(const rome_clique_upsolve_host* u, const int (&nv)[3], int N, UpsolveIndex& X) {
  const rome_clique_host* q = &u->clique;
  if (N > ROME_MAX_PARTICLES_GIBBS) return ROME_ERR_UNSUPPORTED_N;   // the multiscale Gibbs product: lane = output sample, two wavefronts per variable
  if (N < 2 || u->n_up < 0 || (u->n_up > 0 && (!u->up_type || !u->up_var))) return ROME_ERR_INVALID_ARG;
  if (u->schedule != ROME_UPSOLVE_SEQUENTIAL && u->schedule != ROME_UPSOLVE_JACOBI) return ROME_ERR_INVALID_ARG;
  if (q->n_pose2 > nv[0] || q->n_point2 > nv[1] || q->n_pose3 > nv[2]) return ROME_ERR_INVALID_ARG;
  X = UpsolveIndex{};
  X.n_up = u->n_up; X.has_mirror = u->up_mirror != nullptr; X.has_upstream = u->up_stream != nullptr;
  // ---- update list: (type, variable) -> position k in the list, and its position within the type's list
  std::vector<int> kpos[3];
  for (int t = 0; t < 3; ++t) kpos[t].assign((size_t)nv[t], -1);
  X.up_cnt_before.assign((size_t)u->n_up * 3 + 3, 0);
  for (int k = 0; k < u->n_up; ++k) {
    const int t = u->up_type[k], v = u->up_var[k];
    if (t < 0 || t > 2 || v < 0 || v >= nv[t] || kpos[t][v] >= 0) return ROME_ERR_INVALID_ARG;
    if (u->up_stream && (u->up_stream[k] < 0 || u->up_stream[k] >= (1 << 28))) return ROME_ERR_INVALID_ARG;
    if (u->up_mirror && u->up_mirror[k] < -1) return ROME_ERR_INVALID_ARG;
    kpos[t][v] = k;
    for (int tt = 0; tt < 3; ++tt) X.up_cnt_before[3 * (size_t)(k + 1) + tt] = X.up_cnt_before[3 * (size_t)k + tt] + (tt == t ? 1 : 0);
    TypeIndex& x = X.type[t];
    const int pos = x.n_up++;
    x.up.push_back(k);
    x.block.push_back(v);
    x.stream.push_back(u->up_stream ? u->up_stream[k] : pos);
    x.mirror.push_back(u->up_mirror ? u->up_mirror[k] : -1);
    for (int e : {kVdim[t], v, pos, t}) x.gather.push_back(e);
  }
  auto pos_in_type = [&](int k, int t) { return (size_t)X.up_cnt_before[3 * (size_t)k + t]; };
  // ---- the proposal buffer of every type: family rows, host messages, store-resident messages
  make_fams(q, X.fam);
  int rc;
  for (const Fam& f : X.fam) { if ((rc = check_fam_rows(f, nv))) return rc; X.type[f.vt].prop_rows += f.n; }
  const int n_msg[3] = {u->n_msg_pose2, u->n_msg_point2, u->n_msg_pose3}, n_smsg[3] = {u->n_smsg_pose2, u->n_smsg_point2, u->n_smsg_pose3};
  const double* msg[3] = {u->msg_pose2, u->msg_point2, u->msg_pose3};
  const int32_t* msg_up[3] = {u->msg_pose2_up, u->msg_point2_up, u->msg_pose3_up};
  const int32_t* smsg_src[3] = {u->smsg_pose2_src, u->smsg_point2_src, u->smsg_pose3_src};
  const int32_t* smsg_up[3] = {u->smsg_pose2_up, u->smsg_point2_up, u->smsg_pose3_up};
  for (int t = 0; t < 3; ++t) {
    TypeIndex& x = X.type[t];
    if (n_msg[t] < 0 || (n_msg[t] > 0 && (!msg[t] || !msg_up[t]))) return ROME_ERR_INVALID_ARG;
    if (n_smsg[t] < 0 || (n_smsg[t] > 0 && (!smsg_src[t] || !smsg_up[t]))) return ROME_ERR_INVALID_ARG;
    x.n_msg = n_msg[t]; x.msg_base = x.prop_rows; x.prop_rows += n_msg[t];
    x.n_smsg = n_smsg[t]; x.smsg_base = x.prop_rows; x.prop_rows += n_smsg[t];
  }
  // ---- rows: every row targets an updated variable, rows grouped in update order; the row range of every update position; CSR
  std::vector<std::vector<int32_t>> csr[3];   // per type: proposal rows of every updated variable
  for (int t = 0; t < 3; ++t) csr[t].resize(X.type[t].up.size());
  for (int k4 = 0; k4 < NF; ++k4) {
    const Fam& f = X.fam[k4];
    X.fam_lo[k4].assign((size_t)u->n_up + 1, 0);
    int prev = -1;
    for (int r = 0; r < f.n; ++r) {
      const int k = kpos[f.vt][f.rows4[4 * (size_t)r + 3]];
      if (k < 0 || k < prev) return ROME_ERR_INVALID_ARG;
      for (int kk = prev + 1; kk <= k; ++kk) X.fam_lo[k4][kk] = r;
      prev = k;
      csr[f.vt][pos_in_type(k, f.vt)].push_back(f.base + r);
    }
    for (int kk = prev + 1; kk <= u->n_up; ++kk) X.fam_lo[k4][kk] = f.n;
  }
  for (int t = 0; t < 3; ++t)
    for (int m = 0; m < n_msg[t]; ++m) {
      const int k = msg_up[t][m];
      if (k < 0 || k >= u->n_up || u->up_type[k] != t) return ROME_ERR_INVALID_ARG;
      csr[t][pos_in_type(k, t)].push_back(X.type[t].msg_base + m);
    }
  for (int t = 0; t < 3; ++t)
    for (int m = 0; m < n_smsg[t]; ++m) {   // store-resident messages: source = a block of the store that this plan does not write
      const int k = smsg_up[t][m], src = smsg_src[t][m], row = X.type[t].smsg_base + m;
      if (k < 0 || k >= u->n_up || u->up_type[k] != t || src < 0 || src >= nv[t] || kpos[t][src] >= 0) return ROME_ERR_INVALID_ARG;
      csr[t][pos_in_type(k, t)].push_back(row);
      for (int e : {kVdim[t], src, row, t}) X.type[t].smsg.push_back(e);
    }
  for (int t = 0; t < 3; ++t) {
    TypeIndex& x = X.type[t];
    x.ptr.push_back(0);
    for (const auto& l : csr[t]) {
      x.rows.insert(x.rows.end(), l.begin(), l.end());
      x.ptr.push_back((int32_t)x.rows.size());
      if ((int)l.size() > x.max_k) x.max_k = (int)l.size();
    }
    if (x.rows.empty()) x.rows.push_back(0);
  }
  // ---- steps: ranges [k0, k1) of the update list that are updated together
  X.step_k.push_back(0);
  if (u->up_group) {
    for (int k = 1; k < u->n_up; ++k) {
      if (u->up_group[k] < u->up_group[k - 1]) return ROME_ERR_INVALID_ARG;
      if (u->up_group[k] != u->up_group[k - 1]) X.step_k.push_back(k);
    }
  } else if (u->schedule == ROME_UPSOLVE_SEQUENTIAL) {
    for (int k = 1; k < u->n_up; ++k) X.step_k.push_back(k);
  }
  X.step_k.push_back(u->n_up);
  return ROME_OK;
}

/* ---- arenas ---- */
// One pass over an arena.  take(bytes) reserves the next piece, put(src, bytes) reserves it and owes it a copy; every piece starts on a
// 256-byte boundary.  A default-constructed cursor MEASURES: it only adds up (`used` is the arena's size) and hands out nullptr.  A cursor
// over an allocation of that size PLACES: it hands out the pieces and lists the copies, which commit() has the caller perform -- after
// checking that the pass used exactly the bytes that were measured, so that no copy is issued into an arena that does not fit.
struct ArenaCursor {
  struct Copy { void* dst; const void* src; size_t bytes; };
  unsigned char* base = nullptr;
  size_t cap = 0, used = 0;
  std::vector<Copy> copies;
  ArenaCursor() = default;
  ArenaCursor(void* arena, size_t bytes) : base((unsigned char*)arena), cap(bytes) {}
  bool placing() const { return base != nullptr; }
  void* take(size_t bytes) { void* p = base ? base + used : nullptr; used += al256(bytes); return p; }
  void* put(const void* src, size_t bytes) {
    void* p = take(bytes);
    if (p && bytes) copies.push_back({p, src, bytes});
    return p;
  }
  template <class T> T* put(const std::vector<T>& v) { return (T*)put(v.data(), v.size() * sizeof(T)); }
  // copy(dst, src, bytes) -> ROME_OK or an error code; the sources must stay until the copies have completed
  template <class F> int commit(F&& copy) const {
    if (used != cap) return ROME_ERR_ALLOC;   // (unreachable: both passes run the same layout function)
    for (const Copy& c : copies) if (int rc = copy(c.dst, c.src, c.bytes)) return rc;
    return ROME_OK;
  }
};

// the belief blocks of the three variable types, [nv][dim][N] SoA each: the temporary store of the one-shot up-solve
inline void lay_beliefs(ArenaCursor& a, const int (&nv)[3], int N, double* (&bel)[3]) {
  for (int t = 0; t < 3; ++t) bel[t] = (double*)a.take((size_t)nv[t] * kVdim[t] * N * 8);
}
// a family's device tables (rows4, mu, L, the optional columns).  MvNormal factors get the packed Cholesky factor of every covariance,
// computed into `Ls` by the placing pass only (`Ls` is a copy's source)
struct FamDev { const int32_t* rows = nullptr; const double* mu = nullptr; const double* L = nullptr; const int32_t* alt = nullptr;
                const double* hw = nullptr; const double* nh = nullptr; const int32_t* sid = nullptr; const int32_t* meas = nullptr; };
inline int lay_fam(ArenaCursor& a, const Fam& f, std::vector<double>& Ls, FamDev& d) {
  d = FamDev{};
  if (f.n == 0) return ROME_OK;
  const double* Lsrc = f.spread;
  if (f.kind != 1 && a.placing()) {
    Ls.resize((size_t)f.F * f.nL);
    if (int rc = rome_cholesky_lower(f.dz, f.F, f.spread, Ls.data())) return rc;
    Lsrc = Ls.data();
  }
  d.rows = (const int32_t*)a.put(f.rows4, (size_t)f.n * 16);
  d.mu = (const double*)a.put(f.mu, (size_t)f.F * f.dz * 8);
  d.L = (const double*)a.put(Lsrc, (size_t)f.F * f.nL * 8);
  if (f.alt) { d.alt = (const int32_t*)a.put(f.alt, (size_t)f.n * 4); d.hw = (const double*)a.put(f.hw, (size_t)f.n * 8); }
  if (f.nh) d.nh = (const double*)a.put(f.nh, (size_t)f.n * 8);
  if (f.sid) d.sid = (const int32_t*)a.put(f.sid, (size_t)f.n * 4);
  if (f.meas) d.meas = (const int32_t*)a.put(f.meas, (size_t)f.n * 4);
  return ROME_OK;
}
// the arena of rome_clique_proposals: belief blocks, then every family's tables and its output blocks [n][dt][N]
struct ProposalsArena { double* bel[3]; FamDev fd[NF]; double* out[NF]; };
inline int lay_proposals(ArenaCursor& a, const Fam (&fam)[NF], const int (&nv)[3], int N, std::vector<double> (&Ls)[NF], ProposalsArena& A) {
  lay_beliefs(a, nv, N, A.bel);
  for (int k = 0; k < NF; ++k) {
    if (int rc = lay_fam(a, fam[k], Ls[k], A.fd[k])) return rc;
    A.out[k] = (double*)a.take((size_t)fam[k].n * fam[k].dt * N * 8);
  }
  return ROME_OK;
}
// the arena of an up-solve plan: per type the proposal buffer [prop_rows][dim][N] and its bandwidths, the download buffers of the new
// beliefs and their bandwidths, and the index tables; then every family's tables
struct TypeDev {
  double* prop = nullptr; double* pbw = nullptr; double* newout = nullptr; double* bwout = nullptr;
  int32_t* ptr = nullptr; int32_t* rows = nullptr; int32_t* block = nullptr; int32_t* stream = nullptr; int32_t* mirror = nullptr;
  int32_t* gather = nullptr; int32_t* smsg = nullptr;
};
template <class TypeRecord>   // (TypeDev or a record derived from it)
int lay_plan(ArenaCursor& a, const UpsolveIndex& X, int N, std::vector<double> (&Ls)[NF], TypeRecord (&dev)[3], FamDev (&fd)[NF]) {
  for (int t = 0; t < 3; ++t) {
    const TypeIndex& x = X.type[t];
    TypeDev& d = dev[t];
    const size_t blk = (size_t)kVdim[t] * N * 8, bw = (size_t)kVdim[t] * 8;
    d.prop = (double*)a.take(x.prop_rows * blk); d.pbw = (double*)a.take(x.prop_rows * bw);
    d.newout = (double*)a.take(x.n_up * blk); d.bwout = (double*)a.take(x.n_up * bw);
    d.ptr = a.put(x.ptr); d.rows = a.put(x.rows); d.block = a.put(x.block); d.stream = a.put(x.stream); d.mirror = a.put(x.mirror);
    d.gather = a.put(x.gather); d.smsg = a.put(x.smsg);
  }
  for (int k = 0; k < NF; ++k) if (int rc = lay_fam(a, X.fam[k], Ls[k], fd[k])) return rc;
  return ROME_OK;
}

}  // namespace rome
