// rome_capi_clique.hip -- the clique batch, the device-resident belief store and the three plan kinds (up-solve, scatter, block operations)
// behind the extern "C" boundary of librome_mi355.so.  Host-side plumbing only.
#include "rome_capi_internal.h"

using namespace rome;

/* ---- clique-level batch from host beliefs ---- */
namespace {
// the five row families of a rome_clique_host.  kind: 0 Pose2Pose2 (+ PriorPose2 rows), 1 bearing-range, 2 Pose3Pose3 (+ PriorPose3 rows),
// 3 PriorPoint2 sampler; variable types: 0 Pose2, 1 Point2, 2 Pose3; valt = type of the array an `alt` entry indexes (-1: no multihypo);
// base = first row of the family in the proposal buffer of its target type (rome_clique_upsolve)
struct Fam {
  int n; const int32_t* rows4; int F; const double* mu; const double* spread; int dz, nL, dfx, dt; double* out; int vf, vt; int dir_all;
  uint64_t off; int kind; int base;
  const int32_t* alt; const double* hw; const double* nh; const int32_t* sid; int valt;
  const int32_t* meas;   // per-row block of the measurement samples (Pose2Pose2 / bearing-range / Pose3Pose3 rows), or nullptr
  int vmeas() const { return kind == 1 ? 1 : (kind == 2 ? 2 : 0); }   // variable type of the store array a `meas` entry indexes
};
constexpr int NF = 5;
void make_fams(const rome_clique_host* q, Fam (&fam)[NF]) {
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
int check_fam_rows(const Fam& f, const int (&nv)[3]) {
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
// bytes of a family's device tables (rows4, mu, L, the optional columns)
size_t fam_table_bytes(const Fam& f) {
  return al256((size_t)f.n * 16) + al256((size_t)f.F * f.dz * 8) + al256((size_t)f.F * f.nL * 8) + 256 +
         (f.alt ? al256((size_t)f.n * 4) + al256((size_t)f.n * 8) : 0) + (f.nh ? al256((size_t)f.n * 8) : 0) + (f.sid ? al256((size_t)f.n * 4) : 0) +
         (f.meas ? al256((size_t)f.n * 4) : 0);
}
struct FamDev { const int32_t* rows = nullptr; const double* mu = nullptr; const double* L = nullptr; const int32_t* alt = nullptr;
                const double* hw = nullptr; const double* nh = nullptr; const int32_t* sid = nullptr; const int32_t* meas = nullptr; };
// uploads a family's tables into `arena` (asynchronously: `Ls` must outlive the stream work); MvNormal factors get their packed Cholesky
int upload_fam(rome_ctx* c, const Fam& f, unsigned char* arena, size_t* used, std::vector<double>& Ls, FamDev& d) {
  d = FamDev{};
  if (f.n == 0) return ROME_OK;
  hipStream_t s = c->stream;
  const double* Lsrc = f.spread;
  int rc;
  if (f.kind != 1) {   // MvNormal factors: packed lower Cholesky of every covariance
    Ls.resize((size_t)f.F * f.nL);
    if ((rc = rome_cholesky_lower(f.dz, f.F, f.spread, Ls.data()))) return rc;
    Lsrc = Ls.data();
  }
  auto put = [&](const void* src, size_t bytes) -> void* {
    void* dst = arena + *used;
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return nullptr;
    *used += al256(bytes);
    return dst;
  };
#define ROME_PUT(dst, T, src, bytes) do { void* _p = put((src), (bytes)); if (!_p) return hip_fail(c, hipGetLastError()); (dst) = (const T*)_p; } while (0)
  ROME_PUT(d.rows, int32_t, f.rows4, (size_t)f.n * 16);
  ROME_PUT(d.mu, double, f.mu, (size_t)f.F * f.dz * 8);
  ROME_PUT(d.L, double, Lsrc, (size_t)f.F * f.nL * 8);
  if (f.alt) { ROME_PUT(d.alt, int32_t, f.alt, (size_t)f.n * 4); ROME_PUT(d.hw, double, f.hw, (size_t)f.n * 8); }
  if (f.nh) ROME_PUT(d.nh, double, f.nh, (size_t)f.n * 8);
  if (f.sid) ROME_PUT(d.sid, int32_t, f.sid, (size_t)f.n * 4);
  if (f.meas) ROME_PUT(d.meas, int32_t, f.meas, (size_t)f.n * 4);
#undef ROME_PUT
  return ROME_OK;
}
// rows [lo, hi) of a family: one convolution launch into `out` (the block of row `lo`)
hipError_t launch_fam(const Fam& f, const FamDev& d, const rome_opts* o, uint64_t stream_base, int lo, int hi, const double* bel_fixed,
                      const double* bel_target, double* out, hipStream_t s, const double* meas_base = nullptr) {
  ConvArgs a;
  rome_opts of = *o;
  of.stream_offset = stream_base + f.off + (d.sid ? 0ull : (uint64_t)lo);   // family offsets of the device graph (DeviceGraph.STREAM_*)
  fill_args(a, &of);
  a.n_conv = hi - lo; a.dir_all = f.dir_all; a.rows4 = d.rows + 4 * (size_t)lo;
  a.mu = d.mu; a.L = d.L;
  a.bel_fixed = bel_fixed; a.bel_target = bel_target; a.out = out;
  a.alt_var = d.alt ? d.alt + lo : nullptr; a.hypo_w = d.alt ? d.hw + lo : nullptr;
  a.nullhypo = d.nh ? d.nh + lo : nullptr;
  a.row_stream = d.sid ? d.sid + lo : nullptr;
  if (d.meas && meas_base) { a.meas_block = d.meas + lo; a.meas_base = meas_base; }
  return f.kind == 0 ? launch_conv_pose2pose2(a, o->solver, s) : (f.kind == 1 ? launch_conv_bearingrange(a, o->solver, s)
                     : (f.kind == 2 ? launch_conv_pose3pose3(a, o->solver, s) : launch_sample_priorpoint2(a, s)));
}
}  // namespace

extern "C" {

int rome_clique_proposals(rome_ctx* c, const rome_opts* o, const rome_clique_host* q) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || !q) return ROME_ERR_INVALID_ARG;
  const int N = o->n_particles;
  Fam fam[NF]; make_fams(q, fam);
  const int nv[3] = {q->n_pose2, q->n_point2, q->n_pose3};
  const int vdim[3] = {3, 2, 6};
  const double* vhost[3] = {q->bel_pose2, q->bel_point2, q->bel_pose3};
  size_t need = 0;
  for (int t = 0; t < 3; ++t) { if (nv[t] < 0 || (nv[t] > 0 && !vhost[t])) return ROME_ERR_INVALID_ARG; need += al256((size_t)nv[t] * vdim[t] * N * 8); }
  for (const Fam& f : fam) {
    if ((rc = check_fam_rows(f, nv))) return rc;
    if (f.n > 0 && !f.out) return ROME_ERR_INVALID_ARG;
    if (f.meas) return ROME_ERR_INVALID_ARG;   // measurement-sample rows address a store (rome_upsolve_plan)
    need += al256((size_t)f.n * f.dt * N * 8) + fam_table_bytes(f);
  }
  ROME_BIND(c);
  void* arena_v = nullptr;
  if ((rc = ensure(c, 9, need + 4096, &arena_v))) return rc;
  unsigned char* arena = (unsigned char*)arena_v;
  size_t used = 0;
  double* dbel[3];
  for (int t = 0; t < 3; ++t) {
    dbel[t] = (double*)(arena + used);
    if ((rc = stage_blocks(c, o->layout, nv[t], vdim[t], N, vhost[t], dbel[t]))) return rc;
    used += al256((size_t)nv[t] * vdim[t] * N * 8);
  }
  hipStream_t s = c->stream;
  std::vector<std::vector<double>> Ls(NF);
  DrainOnExit drain{s};
  double* dout[NF] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < NF; ++k) {
    const Fam& f = fam[k];
    if (f.n == 0) continue;
    FamDev d;
    if ((rc = upload_fam(c, f, arena, &used, Ls[k], d))) return rc;
    dout[k] = (double*)(arena + used);
    used += al256((size_t)f.n * f.dt * N * 8);
    ROME_HIP(c, launch_fam(f, d, o, o->stream_offset, 0, f.n, dbel[f.vf], dbel[f.vt], dout[k], s));
  }
  // proposals back to the host in the caller's layout
  for (int k = 0; k < NF; ++k)
    if ((rc = fetch_blocks(c, o->layout, fam[k].n, fam[k].dt, N, dout[k], fam[k].out))) return rc;
  return ROME_OK;
}

}  // extern "C"

/* ---- belief store + up-solve plans: gibbs_iters x {proposals -> manikde! bandwidths -> multiscale Gibbs product -> in-place write},
 *      device-resident across calls ---- */
struct rome_store {
  rome_ctx* ctx = nullptr;
  int N = 0;
  int nv[3] = {0, 0, 0};
  double* bel[3] = {nullptr, nullptr, nullptr};
  DevBuf own[3];   // what bel[] points into (empty for a store that wraps the caller's arrays)
};
struct rome_scatter_plan {
  rome_ctx* ctx = nullptr; rome_store* st = nullptr;
  int n = 0; int64_t stride = 0;
  DevBuf ent;   // int32 [n][4] = (dim, var, src_block, type)
};
struct rome_blockop_plan {
  rome_ctx* ctx = nullptr; rome_store* st = nullptr;
  int op = 0, n = 0;
  int n_lo = 0;  // entries [0, n_lo) run in k_block_ops, [n_lo, n) in k_block_ops_pose3 (COMPOSE on Pose3 blocks: 0; ANCHOR_MEAN: its Pose2 / Point2 entries first)
  DevBuf ent;   // int32 [n][4] = (type, a, b, dst)
  DevBuf prm;   // COMPOSE: double [n][2] = (translation, heading) inflation of the composed deviations, or empty
};
struct rome_upsolve_plan {
  rome_ctx* ctx = nullptr; rome_store* st = nullptr;
  int N = 0, layout = 0, gi = 3, pi = 1, n_up = 0;
  Fam fam[NF]; FamDev fd[NF];
  std::vector<int> fam_lo[NF];            // first row of family f that targets update position >= k (rows are grouped in update order)
  std::vector<int> step_k;                // boundaries of the update steps (ranges of the update list updated together)
  std::vector<int> up_cnt_before;         // [k][t]: updates of type t among the first k
  int n_upt[3] = {0, 0, 0}, prop_rows_t[3] = {0, 0, 0}, max_k[3] = {1, 1, 1};
  double* d_prop[3] = {nullptr, nullptr, nullptr}; double* d_pbw[3] = {nullptr, nullptr, nullptr};
  int32_t* d_ptr[3] = {nullptr, nullptr, nullptr}; int32_t* d_rws[3] = {nullptr, nullptr, nullptr};
  int32_t* d_upblock[3] = {nullptr, nullptr, nullptr}; int32_t* d_upstream[3] = {nullptr, nullptr, nullptr};
  int32_t* d_upmirror[3] = {nullptr, nullptr, nullptr};
  int32_t* d_gather[3] = {nullptr, nullptr, nullptr};   // (dim, var, position, type) per updated variable: store -> contiguous download buffer
  double* d_newout[3] = {nullptr, nullptr, nullptr}; double* d_bwout[3] = {nullptr, nullptr, nullptr};
  double* new_host[3] = {nullptr, nullptr, nullptr}; double* bw_host[3] = {nullptr, nullptr, nullptr};
  bool has_mirror = false, has_upstream = false;
  int n_smsg[3] = {0, 0, 0}, smsg_base[3] = {0, 0, 0};   // store-resident messages: rows [smsg_base, smsg_base + n_smsg) of the type's proposal buffer
  int32_t* d_smsg_ent[3] = {nullptr, nullptr, nullptr};  // (dim, source block, proposal row, type) per message: gathered at the start of every run
  DevBuf arena;   // the plan's device memory (empty when it is carved from the context's arena: the one-shot host entry)
  size_t tree_need = 8;               // the tree workspaces of the three types side by side (their products may run concurrently)
  size_t tree_off[3] = {0, 0, 0};
};

namespace {
const int kVdim[3] = {3, 2, 6};
const uint32_t kCircBw[3] = {0b100u, 0u, 0b111000u}, kCircProd[3] = {0b100u, 0u, 0u};
const uint64_t kProdOff[3] = {3ull << 28, 4ull << 28, 6ull << 28};

// builds a plan over `st`; ctx_arena: carve the plan's device memory from the context's arena (the one-shot host entry) instead of an
// allocation the plan owns
int plan_build(rome_ctx* c, rome_store* st, const rome_opts* o, const rome_clique_upsolve_host* u, rome_upsolve_plan* P, bool ctx_arena) {
  const rome_clique_host* q = &u->clique;
  const int N = o->n_particles;
  if (N > ROME_MAX_PARTICLES_GIBBS) return ROME_ERR_UNSUPPORTED_N;   // the multiscale Gibbs product: lane = output sample, two wavefronts per variable
  if (N != st->N) return ROME_ERR_INVALID_ARG;
  if (N < 2 || u->n_up < 0 || (u->n_up > 0 && (!u->up_type || !u->up_var))) return ROME_ERR_INVALID_ARG;
  if (u->schedule != ROME_UPSOLVE_SEQUENTIAL && u->schedule != ROME_UPSOLVE_JACOBI) return ROME_ERR_INVALID_ARG;
  P->ctx = c; P->st = st; P->N = N; P->layout = o->layout; P->n_up = u->n_up;
  P->gi = u->gibbs_iters > 0 ? u->gibbs_iters : 3; P->pi = u->product_iters > 0 ? u->product_iters : 1;
  const int nv[3] = {st->nv[0], st->nv[1], st->nv[2]};
  if (q->n_pose2 > nv[0] || q->n_point2 > nv[1] || q->n_pose3 > nv[2]) return ROME_ERR_INVALID_ARG;
  // ---- update list: (type, variable) -> global position k and position within the type's list
  std::vector<int> kpos[3], uplist[3];
  for (int t = 0; t < 3; ++t) kpos[t].assign((size_t)nv[t], -1);
  P->up_cnt_before.assign((size_t)u->n_up * 3 + 3, 0);
  for (int k = 0; k < u->n_up; ++k) {
    const int t = u->up_type[k], v = u->up_var[k];
    if (t < 0 || t > 2 || v < 0 || v >= nv[t] || kpos[t][v] >= 0) return ROME_ERR_INVALID_ARG;
    if (u->up_stream && (u->up_stream[k] < 0 || u->up_stream[k] >= (1 << 28))) return ROME_ERR_INVALID_ARG;
    if (u->up_mirror && u->up_mirror[k] < -1) return ROME_ERR_INVALID_ARG;
    kpos[t][v] = k;
    for (int tt = 0; tt < 3; ++tt) P->up_cnt_before[3 * (size_t)(k + 1) + tt] = P->up_cnt_before[3 * (size_t)k + tt] + (tt == t ? 1 : 0);
    uplist[t].push_back(k);
  }
  make_fams(q, P->fam);
  const int n_msg[3] = {u->n_msg_pose2, u->n_msg_point2, u->n_msg_pose3};
  const double* msg_host[3] = {u->msg_pose2, u->msg_point2, u->msg_pose3};
  const int32_t* msg_up[3] = {u->msg_pose2_up, u->msg_point2_up, u->msg_pose3_up};
  double* new_host[3] = {u->new_pose2, u->new_point2, u->new_pose3};
  double* bw_host[3] = {u->bw_pose2, u->bw_point2, u->bw_pose3};
  const int n_smsg[3] = {u->n_smsg_pose2, u->n_smsg_point2, u->n_smsg_pose3};
  const int32_t* smsg_src[3] = {u->smsg_pose2_src, u->smsg_point2_src, u->smsg_pose3_src};
  const int32_t* smsg_up[3] = {u->smsg_pose2_up, u->smsg_point2_up, u->smsg_pose3_up};
  int msg_base[3];
  int rc;
  for (int t = 0; t < 3; ++t) P->prop_rows_t[t] = 0;
  for (const Fam& f : P->fam) { if ((rc = check_fam_rows(f, nv))) return rc; P->prop_rows_t[f.vt] += f.n; }
  for (int t = 0; t < 3; ++t) {
    if (n_msg[t] < 0 || (n_msg[t] > 0 && (!msg_host[t] || !msg_up[t]))) return ROME_ERR_INVALID_ARG;
    P->n_upt[t] = (int)uplist[t].size();
    P->new_host[t] = P->n_upt[t] ? new_host[t] : nullptr; P->bw_host[t] = P->n_upt[t] ? bw_host[t] : nullptr;
    msg_base[t] = P->prop_rows_t[t]; P->prop_rows_t[t] += n_msg[t];
    if (n_smsg[t] < 0 || (n_smsg[t] > 0 && (!smsg_src[t] || !smsg_up[t]))) return ROME_ERR_INVALID_ARG;
    P->n_smsg[t] = n_smsg[t]; P->smsg_base[t] = P->prop_rows_t[t]; P->prop_rows_t[t] += n_smsg[t];
  }
  P->has_mirror = u->up_mirror != nullptr; P->has_upstream = u->up_stream != nullptr;
  // ---- rows: every row targets an updated variable, rows grouped in update order; the row range of every update position; CSR
  std::vector<std::vector<int>> csr[3];    // per type: proposal rows (in the type's buffer) of every updated variable, in update order
  for (int t = 0; t < 3; ++t) csr[t].resize(uplist[t].size());
  for (int k4 = 0; k4 < NF; ++k4) {
    const Fam& f = P->fam[k4];
    P->fam_lo[k4].assign((size_t)u->n_up + 1, 0);
    int prev = -1;
    for (int r = 0; r < f.n; ++r) {
      const int32_t* e = f.rows4 + 4 * (size_t)r;
      const int k = kpos[f.vt][e[3]];
      if (k < 0 || k < prev) return ROME_ERR_INVALID_ARG;
      if (k != prev) { for (int kk = prev + 1; kk <= k; ++kk) P->fam_lo[k4][kk] = r; }
      prev = k;
      csr[f.vt][(size_t)(P->up_cnt_before[3 * (size_t)k + f.vt])].push_back(f.base + r);
    }
    for (int kk = prev + 1; kk <= u->n_up; ++kk) P->fam_lo[k4][kk] = f.n;
  }
  for (int t = 0; t < 3; ++t)
    for (int m = 0; m < n_msg[t]; ++m) {
      const int k = msg_up[t][m];
      if (k < 0 || k >= u->n_up || u->up_type[k] != t) return ROME_ERR_INVALID_ARG;
      csr[t][(size_t)P->up_cnt_before[3 * (size_t)k + t]].push_back(msg_base[t] + m);
    }
  std::vector<int32_t> sm_h[3];
  for (int t = 0; t < 3; ++t)
    for (int m = 0; m < n_smsg[t]; ++m) {   // store-resident messages: source = a block of the store that this plan does not write
      const int k = smsg_up[t][m], src = smsg_src[t][m];
      if (k < 0 || k >= u->n_up || u->up_type[k] != t || src < 0 || src >= nv[t] || kpos[t][src] >= 0) return ROME_ERR_INVALID_ARG;
      csr[t][(size_t)P->up_cnt_before[3 * (size_t)k + t]].push_back(P->smsg_base[t] + m);
      sm_h[t].push_back(kVdim[t]); sm_h[t].push_back(src); sm_h[t].push_back(P->smsg_base[t] + m); sm_h[t].push_back(t);
    }
  std::vector<int32_t> ptr_h[3], rws_h[3], blk_h[3], sid_h[3], mir_h[3], gat_h[3];
  for (int t = 0; t < 3; ++t) {
    P->max_k[t] = 1;
    ptr_h[t].push_back(0);
    for (const auto& l : csr[t]) { for (int r : l) rws_h[t].push_back(r); ptr_h[t].push_back((int32_t)rws_h[t].size()); if ((int)l.size() > P->max_k[t]) P->max_k[t] = (int)l.size(); }
    if (rws_h[t].empty()) rws_h[t].push_back(0);
    int pos = 0;
    for (int k : uplist[t]) {
      blk_h[t].push_back(u->up_var[k]);
      sid_h[t].push_back(u->up_stream ? u->up_stream[k] : pos);
      mir_h[t].push_back(u->up_mirror ? u->up_mirror[k] : -1);
      gat_h[t].push_back(kVdim[t]); gat_h[t].push_back(u->up_var[k]); gat_h[t].push_back(pos); gat_h[t].push_back(t);
      ++pos;
    }
  }
  // ---- steps: ranges [k0, k1) of the update list that are updated together
  P->step_k.clear(); P->step_k.push_back(0);
  if (u->up_group) {
    for (int k = 1; k < u->n_up; ++k) {
      if (u->up_group[k] < u->up_group[k - 1]) return ROME_ERR_INVALID_ARG;
      if (u->up_group[k] != u->up_group[k - 1]) P->step_k.push_back(k);
    }
  } else if (u->schedule == ROME_UPSOLVE_SEQUENTIAL) {
    for (int k = 1; k < u->n_up; ++k) P->step_k.push_back(k);
  }
  P->step_k.push_back(u->n_up);
  // ---- device memory
  size_t need = 4096;
  for (int t = 0; t < 3; ++t) {
    const size_t blk = (size_t)kVdim[t] * N * 8, nu = uplist[t].size();
    need += al256((size_t)P->prop_rows_t[t] * blk) + al256((size_t)P->prop_rows_t[t] * kVdim[t] * 8) + al256(ptr_h[t].size() * 4) + al256(rws_h[t].size() * 4)
          + 3 * al256(nu * 4 + 4) + al256(nu * 16 + 16) + al256(nu * blk) + al256(nu * kVdim[t] * 8) + al256((size_t)n_smsg[t] * 16 + 16);
  }
  for (const Fam& f : P->fam) need += fam_table_bytes(f);
  ROME_BIND(c);
  void* arena_v = nullptr;
  if (ctx_arena) { if ((rc = ensure(c, 12, need, &arena_v))) return rc; }
  else { ROME_HIP(c, P->arena.alloc(need)); arena_v = P->arena.p; }
  unsigned char* arena = (unsigned char*)arena_v;
  size_t used = 0;
  hipStream_t s = c->stream;
  std::vector<std::vector<double>> Ls(NF);
  DrainOnExit drain{s};
  auto put = [&](const void* src, size_t bytes, void** dst) -> int {
    *dst = arena + used;
    if (bytes) ROME_HIP(c, hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, s));
    used += al256(bytes);
    return ROME_OK;
  };
  auto take = [&](size_t bytes) -> void* { void* p = arena + used; used += al256(bytes); return p; };
  for (int t = 0; t < 3; ++t) {
    const size_t blk = (size_t)kVdim[t] * N * 8, nu = uplist[t].size();
    P->d_prop[t] = (double*)take((size_t)P->prop_rows_t[t] * blk);
    P->d_pbw[t] = (double*)take((size_t)P->prop_rows_t[t] * kVdim[t] * 8);
    P->d_newout[t] = (double*)take(nu * blk);
    P->d_bwout[t] = (double*)take(nu * kVdim[t] * 8);
    void* p;
    if ((rc = put(ptr_h[t].data(), ptr_h[t].size() * 4, &p))) return rc; P->d_ptr[t] = (int32_t*)p;
    if ((rc = put(rws_h[t].data(), rws_h[t].size() * 4, &p))) return rc; P->d_rws[t] = (int32_t*)p;
    if ((rc = put(blk_h[t].data(), nu * 4, &p))) return rc; P->d_upblock[t] = (int32_t*)p;
    if ((rc = put(sid_h[t].data(), nu * 4, &p))) return rc; P->d_upstream[t] = (int32_t*)p;
    if ((rc = put(mir_h[t].data(), nu * 4, &p))) return rc; P->d_upmirror[t] = (int32_t*)p;
    if ((rc = put(gat_h[t].data(), nu * 16, &p))) return rc; P->d_gather[t] = (int32_t*)p;
    if ((rc = put(sm_h[t].data(), (size_t)n_smsg[t] * 16, &p))) return rc; P->d_smsg_ent[t] = (int32_t*)p;
    if (n_msg[t] > 0) {   // upward messages: appended to the type's proposal buffer, bandwidths once
      double* mb = P->d_prop[t] + (size_t)msg_base[t] * kVdim[t] * N;
      if ((rc = stage_blocks(c, o->layout, n_msg[t], kVdim[t], N, msg_host[t], mb))) return rc;
      ROME_HIP(c, launch_kde_bandwidth(kVdim[t], n_msg[t], N, mb, kCircBw[t], 1e-2, 1e-6,
                                             P->d_pbw[t] + (size_t)msg_base[t] * kVdim[t], s));
    }
    P->tree_off[t] = t == 0 ? 0 : P->tree_need;
    if (t == 0) P->tree_need = 0;
    P->tree_need += al256(gibbs_workspace_bytes(kVdim[t], P->prop_rows_t[t], (int)nu, N)) + 256;
  }
  for (int k4 = 0; k4 < NF; ++k4) if ((rc = upload_fam(c, P->fam[k4], arena, &used, Ls[k4], P->fd[k4]))) return rc;
  if (used > need) return ROME_ERR_ALLOC;
  // the host tables must not be referenced after creation (the caller's arrays may go away)
  for (Fam& f : P->fam) { f.rows4 = nullptr; f.mu = f.spread = nullptr; f.alt = nullptr; f.hw = f.nh = nullptr; f.sid = nullptr; f.out = nullptr; f.meas = nullptr; }
  return ROME_OK;   // (~DrainOnExit: the uploads have completed before Ls goes away)
}

int plan_run(rome_upsolve_plan* P, const rome_opts* o, double* mirror_out, int64_t mirror_stride) {
  rome_ctx* c = P->ctx; rome_store* st = P->st;
  const int N = P->N;
  int rc;
  if (P->has_mirror && !mirror_out) return ROME_ERR_INVALID_ARG;
  if (mirror_stride == 0) mirror_stride = 6 * (int64_t)N;
  if (P->has_mirror)
    if (mirror_stride < (int64_t)N) return ROME_ERR_INVALID_ARG;   // (a block spans dim * N doubles from its slot: PACKED layouts use stride N)
  ROME_BIND(c);
  void* trees = nullptr;
  if ((rc = ensure(c, 10, P->tree_need, &trees))) return rc;
  hipStream_t s = c->stream;
  // A step is two phases of mutually independent launch chains: (A) per row family {convolutions -> manikde! bandwidths of those
  // proposals} -- they read the store, write disjoint proposal rows --, then (B) per variable type {ball trees -> multiscale Gibbs
  // product} -- each writes its own type's blocks in place.  All of (A) precedes all of (B), and all of (B) the next step's (A): a
  // product of one type overwrites beliefs that another family's convolution reads.  A phase with more than one chain runs its
  // chains on side streams of the context (a small clique or frontier pays the LATENCY of its launches: the landmark product need
  // not wait for the pose product; 1.1 -> 0.6 ms per Gibbs iteration on the 36-pose honeycomb, profiles/r04_small_frontier.txt),
  // and consecutive phases are chained DIRECTLY by events -- every chain of a phase waits for the events of the previous phase's
  // chains, one cross-stream hop, not a join into the context's stream followed by a fork out of it (each hop is 20-40 us of queue
  // latency on this stack); the context's stream is joined once at the end.  A phase with a single chain after work that is
  // already on the context's stream stays there: a Manhattan frontier (one family, one type) never leaves the one stream.
  static const bool no_fork = std::getenv("ROME_UPSOLVE_NO_FORK") != nullptr;   // (A/B measurements: everything on the one stream)
  hipEvent_t* ev_cur = c->ev_side;      // events of the phase whose completion the next phase waits for (when !on_main)
  hipEvent_t* ev_nxt = c->ev_side2;
  int n_cur = 0;
  bool on_main = true;                  // everything issued so far is ordered on the context's stream itself
  auto phase = [&](int n_chain, auto&& launch_chain) -> int {
    if (n_chain == 0) return ROME_OK;
    const bool side = n_chain > 1 && !no_fork;
    int rc2;
    if (side || !on_main) { if ((rc2 = ensure_side(c))) return rc2; }
    if (side && on_main) ROME_HIP(c, hipEventRecord(c->ev_fork, s));
    for (int i = 0; i < n_chain; ++i) {
      hipStream_t sx = side ? c->side[i] : s;
      if (on_main) { if (side) ROME_HIP(c, hipStreamWaitEvent(sx, c->ev_fork, 0)); }
      else for (int e = 0; e < n_cur; ++e) ROME_HIP(c, hipStreamWaitEvent(sx, ev_cur[e], 0));
      if ((rc2 = launch_chain(i, sx))) return rc2;
      if (side) ROME_HIP(c, hipEventRecord(ev_nxt[i], sx));
    }
    if (side) { hipEvent_t* t_ = ev_cur; ev_cur = ev_nxt; ev_nxt = t_; n_cur = n_chain; on_main = false; }
    else on_main = true;
    return ROME_OK;
  };
  // store-resident messages: the source blocks as they are NOW -> their proposal rows, and their manikde! bandwidths (once per run)
  for (int t = 0; t < 3; ++t)
    if (P->n_smsg[t] > 0 && P->gi > 0) {
      ROME_HIP(c, launch_scatter_blocks(P->n_smsg[t], N, P->d_smsg_ent[t], P->d_prop[t], (int64_t)kVdim[t] * N, st->bel[0], st->bel[1], st->bel[2], s, /*to_store=*/0));
      ROME_HIP(c, launch_kde_bandwidth(kVdim[t], P->n_smsg[t], N, P->d_prop[t] + (size_t)P->smsg_base[t] * kVdim[t] * N, kCircBw[t], 1e-2, 1e-6,
                                             P->d_pbw[t] + (size_t)P->smsg_base[t] * kVdim[t], s));
    }
  for (int it = 0; it < P->gi; ++it) {
    const uint64_t base = o->stream_offset + ((uint64_t)it << 32);
    const int nsteps = P->n_up > 0 ? (int)P->step_k.size() - 1 : 0;
    for (int stp = 0; stp < nsteps; ++stp) {
      const int k0 = P->step_k[stp], k1 = P->step_k[stp + 1];
      int fam_a[NF], lo_a[NF], hi_a[NF], naf = 0;
      for (int k4 = 0; k4 < NF; ++k4) {
        const Fam& f = P->fam[k4];
        const int lo = P->fam_lo[k4][k0], hi = f.n == 0 ? 0 : (k1 < P->n_up ? P->fam_lo[k4][k1] : f.n);
        if (hi > lo) { fam_a[naf] = k4; lo_a[naf] = lo; hi_a[naf] = hi; ++naf; }
      }
      int typ_a[3], nat = 0;
      for (int t = 0; t < 3; ++t) {
        const int pa = P->up_cnt_before[3 * (size_t)k0 + t], pb = P->up_cnt_before[3 * (size_t)k1 + t];
        if (pb > pa && P->prop_rows_t[t] > 0) typ_a[nat++] = t;
      }
      rc = phase(naf, [&](int i, hipStream_t sx) -> int {
        const int k4 = fam_a[i], lo = lo_a[i], hi = hi_a[i];
        const Fam& f = P->fam[k4];
        double* out = P->d_prop[f.vt] + (size_t)(f.base + lo) * f.dt * N;
        ROME_HIP(c, launch_fam(f, P->fd[k4], o, base, lo, hi, st->bel[f.vf], st->bel[f.vt], out, sx, st->bel[f.vmeas()]));
        if (P->max_k[f.vt] > 1)   // (a plan whose destinations take ONE proposal each -- sampling a graph's measurements, transporting a belief -- multiplies nothing: no manikde!)
          ROME_HIP(c, launch_kde_bandwidth(f.dt, hi - lo, N, out, kCircBw[f.vt], 1e-2, 1e-6, P->d_pbw[f.vt] + (size_t)(f.base + lo) * f.dt, sx));
        return ROME_OK;
      });
      if (rc) return rc;
      rc = phase(nat, [&](int i, hipStream_t sx) -> int {
        const int t = typ_a[i];
        const int pa = P->up_cnt_before[3 * (size_t)k0 + t], pb = P->up_cnt_before[3 * (size_t)k1 + t];
        // the product writes the new beliefs IN PLACE into the store (a product reads only proposals and its own variable's block)
        GibbsPlace place{P->d_upblock[t] + pa, P->has_upstream ? P->d_upstream[t] + pa : nullptr,
                               (P->has_mirror && mirror_out) ? P->d_upmirror[t] + pa : nullptr, mirror_out, mirror_stride};
        ROME_HIP(c, launch_product_gibbs(kVdim[t], pb - pa, N, P->prop_rows_t[t], P->d_ptr[t] + pa, P->d_rws[t], P->d_prop[t], P->d_pbw[t],
                                               st->bel[t], st->bel[t], (unsigned char*)trees + P->tree_off[t], kCircProd[t], P->pi, P->max_k[t],
                                               o->seed, base + kProdOff[t] + (P->has_upstream ? 0ull : (uint64_t)pa), sx, &place));
        return ROME_OK;
      });
      if (rc) return rc;
    }
  }
  if (!on_main) {   // the one join: everything after the run is ordered after it on the context's stream
    for (int e = 0; e < n_cur; ++e) ROME_HIP(c, hipStreamWaitEvent(s, ev_cur[e], 0));
    on_main = true;
  }
  if (P->has_mirror && P->gi > 0) {
    // updated variables whose product never ran (no proposals at all) still owe their block to the mirror: the product kernel handles
    // K = 0 (copy), so nothing to do here as long as the type has proposal rows; a type without any row keeps its beliefs
    for (int t = 0; t < 3; ++t)
      if (P->n_upt[t] && P->prop_rows_t[t] == 0) {
        GibbsPlace place{P->d_upblock[t], nullptr, P->d_upmirror[t], mirror_out, mirror_stride};
        ROME_HIP(c, launch_product_gibbs(kVdim[t], P->n_upt[t], N, 0, P->d_ptr[t], P->d_rws[t], P->d_prop[t], P->d_pbw[t], st->bel[t], st->bel[t],
                                               (unsigned char*)trees + P->tree_off[t], kCircProd[t], 1, 1, o->seed, 0, s, &place));
      }
  }
  // ---- results (only when the plan was created with host outputs): the updated beliefs and their manikde! bandwidths
  bool sync = false;
  for (int t = 0; t < 3; ++t) {
    const int nu = P->n_upt[t];
    if (nu == 0) continue;
    if (P->bw_host[t]) {
      ROME_HIP(c, launch_kde_bandwidth(kVdim[t], nu, N, st->bel[t], kCircBw[t], 1e-2, 1e-6, P->d_bwout[t], s, P->d_upblock[t]));
      ROME_HIP(c, hipMemcpyAsync(P->bw_host[t], P->d_bwout[t], (size_t)nu * kVdim[t] * 8, hipMemcpyDeviceToHost, s));
      sync = true;
    }
    if (P->new_host[t]) {
      ROME_HIP(c, launch_scatter_blocks(nu, N, P->d_gather[t], P->d_newout[t], (int64_t)kVdim[t] * N, st->bel[0], st->bel[1], st->bel[2], s, /*to_store=*/0));
      if ((rc = fetch_blocks(c, P->layout, nu, kVdim[t], N, P->d_newout[t], P->new_host[t]))) return rc;
    }
  }
  if (sync) ROME_HIP(c, hipStreamSynchronize(s));
  return ROME_OK;
}
}  // namespace

extern "C" {

int rome_store_create(rome_ctx* c, int32_t N, int32_t n_pose2, int32_t n_point2, int32_t n_pose3, rome_store** out) {
  if (!c || !out || N < 1 || N > ROME_MAX_PARTICLES || n_pose2 < 0 || n_point2 < 0 || n_pose3 < 0) return ROME_ERR_INVALID_ARG;
  ROME_BIND(c);
  rome_store* st = new (std::nothrow) rome_store();
  if (!st) return ROME_ERR_ALLOC;
  st->ctx = c; st->N = N; st->nv[0] = n_pose2; st->nv[1] = n_point2; st->nv[2] = n_pose3;
  for (int t = 0; t < 3; ++t) {
    const size_t bytes = (size_t)st->nv[t] * kVdim[t] * N * 8;
    hipError_t e = st->own[t].alloc(bytes);
    st->bel[t] = (double*)st->own[t].p;
    if (e == hipSuccess && bytes) e = hipMemsetAsync(st->bel[t], 0, bytes, c->stream);
    if (e != hipSuccess) { delete st; return hip_fail(c, e); }
  }
  *out = st;
  return ROME_OK;
}
int rome_store_wrap(rome_ctx* c, int32_t N, int32_t n_pose2, double* d2, int32_t n_point2, double* dpt, int32_t n_pose3, double* d3, rome_store** out) {
  if (!c || !out || N < 1 || N > ROME_MAX_PARTICLES || n_pose2 < 0 || n_point2 < 0 || n_pose3 < 0) return ROME_ERR_INVALID_ARG;
  if ((n_pose2 > 0 && !d2) || (n_point2 > 0 && !dpt) || (n_pose3 > 0 && !d3)) return ROME_ERR_INVALID_ARG;
  rome_store* st = new (std::nothrow) rome_store();
  if (!st) return ROME_ERR_ALLOC;
  st->ctx = c; st->N = N; st->nv[0] = n_pose2; st->nv[1] = n_point2; st->nv[2] = n_pose3;
  st->bel[0] = d2; st->bel[1] = dpt; st->bel[2] = d3;
  *out = st;
  return ROME_OK;
}
void rome_store_destroy(rome_store* st) {
  if (!st) return;
  (void)bind_device(st->ctx);
  delete st;
}
int rome_store_upload(rome_store* st, int32_t layout, int32_t type, int32_t first, int32_t count, const double* host) {
  if (!st || type < 0 || type > 2 || first < 0 || count < 0 || (int64_t)first + count > st->nv[type] || (count > 0 && !host)) return ROME_ERR_INVALID_ARG;
  if (layout != ROME_LAYOUT_SOA && layout != ROME_LAYOUT_AOS && layout != ROME_LAYOUT_AOS_POINTS) return ROME_ERR_INVALID_ARG;
  if (count == 0) return ROME_OK;
  rome_ctx* c = st->ctx;
  ROME_BIND(c);
  int rc = stage_blocks(c, layout, count, kVdim[type], st->N, host, st->bel[type] + (size_t)first * kVdim[type] * st->N);
  if (rc) return rc;
  ROME_HIP(c, hipStreamSynchronize(c->stream));   // the caller's array may go away
  return ROME_OK;
}
int rome_store_download(rome_store* st, int32_t layout, int32_t type, int32_t first, int32_t count, double* host) {
  if (!st || type < 0 || type > 2 || first < 0 || count < 0 || (int64_t)first + count > st->nv[type] || (count > 0 && !host)) return ROME_ERR_INVALID_ARG;
  if (layout != ROME_LAYOUT_SOA && layout != ROME_LAYOUT_AOS && layout != ROME_LAYOUT_AOS_POINTS) return ROME_ERR_INVALID_ARG;
  rome_ctx* c = st->ctx;
  ROME_BIND(c);
  return fetch_blocks(c, layout, count, kVdim[type], st->N, st->bel[type] + (size_t)first * kVdim[type] * st->N, host);
}
int rome_store_ptr(rome_store* st, int32_t type, void** dev, int32_t* n_blocks) {
  if (!st || type < 0 || type > 2 || !dev) return ROME_ERR_INVALID_ARG;
  *dev = st->bel[type];
  if (n_blocks) *n_blocks = st->nv[type];
  return ROME_OK;
}

int rome_upsolve_plan_create(rome_ctx* c, rome_store* st, const rome_opts* o, const rome_clique_upsolve_host* u, rome_upsolve_plan** out) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || !st || !u || !out || st->ctx != c) return ROME_ERR_INVALID_ARG;
  rome_upsolve_plan* P = new (std::nothrow) rome_upsolve_plan();
  if (!P) return ROME_ERR_ALLOC;
  rc = plan_build(c, st, o, u, P, false);
  if (rc) { rome_upsolve_plan_destroy(P); return rc; }
  *out = P;
  return ROME_OK;
}
int rome_upsolve_plan_run(rome_upsolve_plan* P, const rome_opts* o, double* mirror_out, int64_t mirror_stride) {
  int rc = check_opts(o); if (rc) return rc;
  if (!P || o->n_particles != P->N || mirror_stride < 0) return ROME_ERR_INVALID_ARG;
  return plan_run(P, o, mirror_out, mirror_stride);
}
void rome_upsolve_plan_destroy(rome_upsolve_plan* P) {
  if (!P) return;
  if (P->ctx) (void)bind_device(P->ctx);   // (ctx is unset when the plan's creation failed its first checks)
  delete P;
}

int rome_scatter_plan_create(rome_ctx* c, rome_store* st, int32_t n, const int32_t* type, const int32_t* var, const int32_t* src_block,
                             int64_t stride, rome_scatter_plan** out) {
  if (!c || !st || st->ctx != c || !out || n < 0 || stride < 0 || (n > 0 && (!type || !var || !src_block))) return ROME_ERR_INVALID_ARG;
  if (stride == 0) stride = 6 * (int64_t)st->N;
  std::vector<int32_t> ent((size_t)n * 4 + 4);
  for (int k = 0; k < n; ++k) {
    const int t = type[k];
    if (t < 0 || t > 2 || var[k] < 0 || var[k] >= st->nv[t] || src_block[k] < 0 || stride < (int64_t)st->N) return ROME_ERR_INVALID_ARG;
    ent[4 * (size_t)k] = kVdim[t]; ent[4 * (size_t)k + 1] = var[k]; ent[4 * (size_t)k + 2] = src_block[k]; ent[4 * (size_t)k + 3] = t;
  }
  ROME_BIND(c);
  rome_scatter_plan* S = new (std::nothrow) rome_scatter_plan();
  if (!S) return ROME_ERR_ALLOC;
  S->ctx = c; S->st = st; S->n = n; S->stride = stride;
  hipError_t e = S->ent.alloc((size_t)n * 16 + 16);
  if (e == hipSuccess && n) e = hipMemcpy(S->ent.p, ent.data(), (size_t)n * 16, hipMemcpyHostToDevice);
  if (e != hipSuccess) { delete S; return hip_fail(c, e); }
  *out = S;
  return ROME_OK;
}
int rome_blockop_plan_create(rome_ctx* c, rome_store* st, int32_t op, int32_t n, const int32_t* type, const int32_t* a, const int32_t* b,
                             const int32_t* dst, rome_blockop_plan** out) {
  return rome_blockop_plan_create_ex(c, st, op, n, type, a, b, dst, nullptr, out);
}
int rome_blockop_plan_create_ex(rome_ctx* c, rome_store* st, int32_t op, int32_t n, const int32_t* type, const int32_t* a, const int32_t* b,
                                const int32_t* dst, const double* params, rome_blockop_plan** out) {
  if (!c || !st || !out || st->ctx != c || n < 0 || op < ROME_BLOCKOP_COPY || op > ROME_BLOCKOP_ANCHOR_MEAN) return ROME_ERR_INVALID_ARG;
  if (params && op != ROME_BLOCKOP_COMPOSE) return ROME_ERR_INVALID_ARG;
  if (params) for (int k = 0; k < 2 * n; ++k) if (!(params[k] > 0.0) || !(params[k] < 1e6)) return ROME_ERR_INVALID_ARG;
  if (n > 0 && (!type || !a || !dst || ((op == ROME_BLOCKOP_RELATIVE || op == ROME_BLOCKOP_COMPOSE) && !b))) return ROME_ERR_INVALID_ARG;
  std::vector<int32_t> ent((size_t)n * 4 + 4, 0);
  for (int k = 0; k < n; ++k) {
    const int t = type[k] & 0xff, fl = type[k] >> 8;
    if (type[k] < 0 || t > 2 || a[k] < 0 || a[k] >= st->nv[op == ROME_BLOCKOP_RELATIVE ? 0 : t] || dst[k] < 0 || dst[k] >= st->nv[t]) return ROME_ERR_INVALID_ARG;
    if (op != ROME_BLOCKOP_COMPOSE && op != ROME_BLOCKOP_MIX && fl != 0) return ROME_ERR_INVALID_ARG;
    if (op == ROME_BLOCKOP_MIX && (fl < 1 || dst[k] == a[k])) return ROME_ERR_INVALID_ARG;
    if (op == ROME_BLOCKOP_RELATIVE && (t > 1 || b[k] < 0 || b[k] >= st->nv[t] || a[k] >= st->nv[0])) return ROME_ERR_INVALID_ARG;
    // (a COMPOSE plan is all-Pose2 or all-Pose3: a run stays one launch)
    if (op == ROME_BLOCKOP_COMPOSE && ((t != 0 && t != 2) || t != (type[0] & 0xff) || fl > 3 || b[k] < 0 || b[k] >= st->nv[t] || dst[k] == a[k] || dst[k] == b[k])) return ROME_ERR_INVALID_ARG;
  }
  // entries of k_block_ops first, those of k_block_ops_pose3 behind them (the entries of a plan are independent: their order is free)
  const bool p3_compose = op == ROME_BLOCKOP_COMPOSE && n > 0 && (type[0] & 0xff) == 2;
  int n_lo = 0;
  for (int k = 0; k < n; ++k) n_lo += !(p3_compose || (op == ROME_BLOCKOP_ANCHOR_MEAN && (type[k] & 0xff) == 2));
  for (int k = 0, lo = 0, hi = n_lo; k < n; ++k) {
    const size_t r = (size_t)((p3_compose || (op == ROME_BLOCKOP_ANCHOR_MEAN && (type[k] & 0xff) == 2)) ? hi++ : lo++);
    ent[4 * r] = type[k]; ent[4 * r + 1] = a[k]; ent[4 * r + 2] = b ? b[k] : 0; ent[4 * r + 3] = dst[k];
  }
  ROME_BIND(c);
  rome_blockop_plan* B = new (std::nothrow) rome_blockop_plan();
  if (!B) return ROME_ERR_ALLOC;
  B->ctx = c; B->st = st; B->op = op; B->n = n; B->n_lo = n_lo;
  hipError_t e = B->ent.alloc((size_t)n * 16 + 16);
  if (e == hipSuccess) e = hipMemcpy(B->ent.p, ent.data(), (size_t)n * 16 + 16, hipMemcpyHostToDevice);
  if (e == hipSuccess && params && n > 0) e = B->prm.alloc((size_t)n * 16);
  if (e == hipSuccess && B->prm.p) e = hipMemcpy(B->prm.p, params, (size_t)n * 16, hipMemcpyHostToDevice);
  if (e != hipSuccess) { delete B; return hip_fail(c, e); }
  *out = B;
  return ROME_OK;
}
int rome_blockop_plan_run(rome_blockop_plan* B) {
  if (!B) return ROME_ERR_INVALID_ARG;
  rome_ctx* c = B->ctx;
  ROME_BIND(c);
  // (ANCHOR_MEAN on Pose2 / Point2 entries IS the anchor of k_block_ops; COMPOSE params belong to one kernel or the other: a plan is one type)
  ROME_HIP(c, launch_block_ops(B->op == ROME_BLOCKOP_ANCHOR_MEAN ? ROME_BLOCKOP_ANCHOR : B->op, B->n_lo, B->st->N, (const int32_t*)B->ent.p, B->st->bel[0],
                               B->st->bel[1], B->st->bel[2], c->stream, (const double*)B->prm.p));
  if (B->n > B->n_lo)
    ROME_HIP(c, launch_block_ops_pose3(B->op, B->n - B->n_lo, B->st->N, (const int32_t*)B->ent.p + 4 * (size_t)B->n_lo, B->st->bel[2], c->stream,
                                       (const double*)B->prm.p));
  return ROME_OK;
}
void rome_blockop_plan_destroy(rome_blockop_plan* B) {
  if (!B) return;
  (void)bind_device(B->ctx);
  delete B;
}

int rome_scatter_plan_run(rome_scatter_plan* S, const double* src_dev) {
  if (!S || (S->n > 0 && !src_dev)) return ROME_ERR_INVALID_ARG;
  rome_ctx* c = S->ctx;
  ROME_BIND(c);
  ROME_HIP(c, launch_scatter_blocks(S->n, S->st->N, (const int32_t*)S->ent.p, src_dev, S->stride, S->st->bel[0], S->st->bel[1], S->st->bel[2], c->stream, 1));
  return ROME_OK;
}
void rome_scatter_plan_destroy(rome_scatter_plan* S) {
  if (!S) return;
  (void)bind_device(S->ctx);
  delete S;
}

/* ---- the one-shot host entry: a temporary store over the clique's host beliefs (context arena) + a plan + one run ---- */
int rome_clique_upsolve(rome_ctx* c, const rome_opts* o, const rome_clique_upsolve_host* u) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || !u) return ROME_ERR_INVALID_ARG;
  const rome_clique_host* q = &u->clique;
  const int N = o->n_particles;
  if (N > ROME_MAX_PARTICLES_GIBBS) return ROME_ERR_UNSUPPORTED_N;
  const int nv[3] = {q->n_pose2, q->n_point2, q->n_pose3};
  const double* vhost[3] = {q->bel_pose2, q->bel_point2, q->bel_pose3};
  size_t need = 4096;
  for (int t = 0; t < 3; ++t) { if (nv[t] < 0 || (nv[t] > 0 && !vhost[t])) return ROME_ERR_INVALID_ARG; need += al256((size_t)nv[t] * kVdim[t] * N * 8); }
  if (u->up_mirror) return ROME_ERR_INVALID_ARG;   // (mirrors belong to plans: there is no device buffer to mirror into here)
  for (int k = 0; k < u->n_up; ++k) {               // the results are read back: every updated type needs its host outputs
    const int t = u->up_type ? u->up_type[k] : -1;
    if (t < 0 || t > 2) return ROME_ERR_INVALID_ARG;
    double* nh[3] = {u->new_pose2, u->new_point2, u->new_pose3}; double* bh[3] = {u->bw_pose2, u->bw_point2, u->bw_pose3};
    if (!nh[t] || !bh[t]) return ROME_ERR_INVALID_ARG;
  }
  ROME_BIND(c);
  void* arena_v = nullptr;
  if ((rc = ensure(c, 11, need, &arena_v))) return rc;
  unsigned char* arena = (unsigned char*)arena_v;
  size_t used = 0;
  rome_store st;
  st.ctx = c; st.N = N;
  {
    DrainOnExit drain{c->stream};
    for (int t = 0; t < 3; ++t) {
      st.nv[t] = nv[t]; st.bel[t] = (double*)(arena + used);
      if ((rc = stage_blocks(c, o->layout, nv[t], kVdim[t], N, vhost[t], st.bel[t]))) return rc;
      used += al256((size_t)nv[t] * kVdim[t] * N * 8);
    }
  }
  rome_upsolve_plan P;
  if ((rc = plan_build(c, &st, o, u, &P, true))) return rc;
  return plan_run(&P, o, nullptr, 0);
}

}  // extern "C"
