// rome_capi_clique.hip -- the clique batch, the device-resident belief store and the three plan kinds (up-solve, scatter, block operations)
// behind the extern "C" boundary of librome_mi355.so.  Host-side plumbing only, and of that only what calls HIP: the row families, the
// validation and update index of an up-solve description and the layout of the three device arenas used here (clique proposals, plan,
// temporary store of the one-shot up-solve) are host-only code in rome_upsolve_index.h.  An arena is never sized by hand: `carve` runs
// its layout function with a measuring cursor, gets memory of exactly that size, runs it again to place, then uploads.
#include "rome_capi_internal.h"

using namespace rome;

/* ---- clique-level batch from host beliefs ---- */
namespace {
// An arena from its layout function `lay(cursor)`: measured, obtained from `memory(bytes, &p)` (-> ROME_OK or an error), placed, and
// the copies it owes issued on the context's stream (asynchronous: their sources must outlive the stream work)
template <class Memory, class Lay> int carve(rome_ctx* c, Memory&& memory, Lay&& lay) {
  ArenaCursor measure;
  (void)lay(measure);
  void* arena = nullptr;
  int rc;
  if ((rc = memory(measure.used, &arena))) return rc;
  ArenaCursor place(arena, measure.used);
  if ((rc = lay(place))) return rc;
  return place.commit([c](void* dst, const void* src, size_t bytes) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    return e == hipSuccess ? ROME_OK : hip_fail(c, e);
  });
}
// the same from workspace `idx` of the context
template <class Lay> int carve_ctx(rome_ctx* c, int idx, Lay&& lay) {
  return carve(c, [=](size_t bytes, void** p) { return ensure(c, idx, bytes, p); }, lay);
}
// the host beliefs of the three variable types (caller's layout) -> their blocks in an arena (lay_beliefs)
int stage_beliefs(rome_ctx* c, int layout, const int (&nv)[3], int N, const double* const (&host)[3], double* const (&bel)[3]) {
  for (int t = 0; t < 3; ++t)
    if (int rc = stage_blocks(c, layout, nv[t], kVdim[t], N, host[t], bel[t])) return rc;
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
  const double* const vhost[3] = {q->bel_pose2, q->bel_point2, q->bel_pose3};
  for (int t = 0; t < 3; ++t) if (nv[t] < 0 || (nv[t] > 0 && !vhost[t])) return ROME_ERR_INVALID_ARG;
  for (const Fam& f : fam) {
    if ((rc = check_fam_rows(f, nv))) return rc;
    if (f.n > 0 && !f.out) return ROME_ERR_INVALID_ARG;
    if (f.meas) return ROME_ERR_INVALID_ARG;   // measurement-sample rows address a store (rome_upsolve_plan)
  }
  ROME_BIND(c);
  std::vector<double> Ls[NF];
  ProposalsArena A;
  hipStream_t s = c->stream;
  DrainOnExit drain{s};
  if ((rc = carve_ctx(c, 9, [&](ArenaCursor& a) { return lay_proposals(a, fam, nv, N, Ls, A); }))) return rc;
  if ((rc = stage_beliefs(c, o->layout, nv, N, vhost, A.bel))) return rc;
  for (int k = 0; k < NF; ++k)
    if (fam[k].n > 0)
      ROME_HIP(c, launch_fam(fam[k], A.fd[k], o, o->stream_offset, 0, fam[k].n, A.bel[fam[k].vf], A.bel[fam[k].vt], A.out[k], s));
  // proposals back to the host in the caller's layout
  for (int k = 0; k < NF; ++k)
    if ((rc = fetch_blocks(c, o->layout, fam[k].n, fam[k].dt, N, A.out[k], fam[k].out))) return rc;
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
  int N = 0, layout = 0, gi = 3, pi = 1;
  UpsolveSteps steps;   // (rome_upsolve_index.h; its family tables point nowhere after creation)
  FamDev fd[NF];
  struct Type : TypeDev, TypeCounts {   // one variable type: its pieces of the arena, its counts, the host outputs (or nullptr), its tree workspace
    double* new_host = nullptr; double* bw_host = nullptr;
    size_t tree_off = 0;
  } type[3];
  DevBuf arena;   // the plan's device memory (empty when it is carved from the context's arena: the one-shot host entry)
  size_t tree_need = 8;   // the tree workspaces of the three types side by side (their products may run concurrently)
};

namespace {
const uint32_t kCircBw[3] = {0b100u, 0u, 0b111000u}, kCircProd[3] = {0b100u, 0u, 0u};
const uint64_t kProdOff[3] = {3ull << 28, 4ull << 28, 6ull << 28};

// builds a plan over `st`: the index (host only), then the arena -- measured, allocated, placed and uploaded by one layout function.
// ctx_arena: carve the plan's device memory from the context's arena (the one-shot host entry) instead of an allocation the plan owns
int plan_build(rome_ctx* c, rome_store* st, const rome_opts* o, const rome_clique_upsolve_host* u, rome_upsolve_plan* P, bool ctx_arena) {
  const int N = o->n_particles;
  if (N > ROME_MAX_PARTICLES_GIBBS) return ROME_ERR_UNSUPPORTED_N;
  if (N != st->N) return ROME_ERR_INVALID_ARG;
  P->ctx = c; P->st = st; P->N = N; P->layout = o->layout;
  P->gi = u->gibbs_iters > 0 ? u->gibbs_iters : 3; P->pi = u->product_iters > 0 ? u->product_iters : 1;
  int rc;
  UpsolveIndex X;   // (its tables feed the uploads: declared before the guard that drains the stream)
  if ((rc = index_upsolve(u, st->nv, N, X))) return rc;
  ROME_BIND(c);
  std::vector<double> Ls[NF];
  hipStream_t s = c->stream;
  DrainOnExit drain{s};   // (the uploads have completed before Ls and the caller's tables go away)
  auto memory = [&](size_t bytes, void** p) -> int {
    if (ctx_arena) return ensure(c, 12, bytes, p);
    ROME_HIP(c, P->arena.alloc(bytes));
    *p = P->arena.p;
    return ROME_OK;
  };
  if ((rc = carve(c, memory, [&](ArenaCursor& a) { return lay_plan(a, X, N, Ls, P->type, P->fd); }))) return rc;
  const double* msg_host[3] = {u->msg_pose2, u->msg_point2, u->msg_pose3};
  double* new_host[3] = {u->new_pose2, u->new_point2, u->new_pose3};
  double* bw_host[3] = {u->bw_pose2, u->bw_point2, u->bw_pose3};
  P->tree_need = 0;
  for (int t = 0; t < 3; ++t) {
    const TypeCounts& x = X.type[t];
    rome_upsolve_plan::Type& y = P->type[t];
    static_cast<TypeCounts&>(y) = x;
    if (x.n_up) { y.new_host = new_host[t]; y.bw_host = bw_host[t]; }
    if (x.n_msg > 0) {   // upward messages: appended to the type's proposal buffer, bandwidths once
      double* mb = y.prop + (size_t)x.msg_base * kVdim[t] * N;
      if ((rc = stage_blocks(c, o->layout, x.n_msg, kVdim[t], N, msg_host[t], mb))) return rc;
      ROME_HIP(c, launch_kde_bandwidth(kVdim[t], x.n_msg, N, mb, kCircBw[t], 1e-2, 1e-6, y.pbw + (size_t)x.msg_base * kVdim[t], s));
    }
    y.tree_off = P->tree_need;
    P->tree_need += al256(gibbs_workspace_bytes(kVdim[t], x.prop_rows, x.n_up, N)) + 256;
  }
  // what a run reads stays with the plan; the host tables must not be referenced after creation (the caller's arrays may go away)
  P->steps = std::move(static_cast<UpsolveSteps&>(X));
  for (Fam& f : P->steps.fam) { f.rows4 = nullptr; f.mu = f.spread = nullptr; f.alt = nullptr; f.hw = f.nh = nullptr; f.sid = nullptr; f.out = nullptr; f.meas = nullptr; }
  return ROME_OK;
}

int plan_run(rome_upsolve_plan* P, const rome_opts* o, double* mirror_out, int64_t mirror_stride) {
  rome_ctx* c = P->ctx; rome_store* st = P->st;
  const UpsolveSteps& X = P->steps;
  const int N = P->N;
  int rc;
  if (X.has_mirror && !mirror_out) return ROME_ERR_INVALID_ARG;
  if (mirror_stride == 0) mirror_stride = 6 * (int64_t)N;
  if (X.has_mirror)
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
  for (int t = 0; t < 3; ++t) {
    const rome_upsolve_plan::Type& y = P->type[t];
    if (y.n_smsg > 0 && P->gi > 0) {
      ROME_HIP(c, launch_scatter_blocks(y.n_smsg, N, y.smsg, y.prop, (int64_t)kVdim[t] * N, st->bel[0], st->bel[1], st->bel[2], s, /*to_store=*/0));
      ROME_HIP(c, launch_kde_bandwidth(kVdim[t], y.n_smsg, N, y.prop + (size_t)y.smsg_base * kVdim[t] * N, kCircBw[t], 1e-2, 1e-6,
                                             y.pbw + (size_t)y.smsg_base * kVdim[t], s));
    }
  }
  for (int it = 0; it < P->gi; ++it) {
    const uint64_t base = o->stream_offset + ((uint64_t)it << 32);
    const int nsteps = X.n_up > 0 ? (int)X.step_k.size() - 1 : 0;
    for (int stp = 0; stp < nsteps; ++stp) {
      const int k0 = X.step_k[stp], k1 = X.step_k[stp + 1];
      int fam_a[NF], lo_a[NF], hi_a[NF], naf = 0;
      for (int k4 = 0; k4 < NF; ++k4) {
        const Fam& f = X.fam[k4];
        const int lo = X.fam_lo[k4][k0], hi = f.n == 0 ? 0 : (k1 < X.n_up ? X.fam_lo[k4][k1] : f.n);
        if (hi > lo) { fam_a[naf] = k4; lo_a[naf] = lo; hi_a[naf] = hi; ++naf; }
      }
      int typ_a[3], nat = 0;
      for (int t = 0; t < 3; ++t) {
        const int pa = X.up_cnt_before[3 * (size_t)k0 + t], pb = X.up_cnt_before[3 * (size_t)k1 + t];
        if (pb > pa && P->type[t].prop_rows > 0) typ_a[nat++] = t;
      }
      rc = phase(naf, [&](int i, hipStream_t sx) -> int {
        const int k4 = fam_a[i], lo = lo_a[i], hi = hi_a[i];
        const Fam& f = X.fam[k4];
        double* out = P->type[f.vt].prop + (size_t)(f.base + lo) * f.dt * N;
        ROME_HIP(c, launch_fam(f, P->fd[k4], o, base, lo, hi, st->bel[f.vf], st->bel[f.vt], out, sx, st->bel[f.vmeas()]));
        if (P->type[f.vt].max_k > 1)   // (a plan whose destinations take ONE proposal each -- sampling a graph's measurements, transporting a belief -- multiplies nothing: no manikde!)
          ROME_HIP(c, launch_kde_bandwidth(f.dt, hi - lo, N, out, kCircBw[f.vt], 1e-2, 1e-6, P->type[f.vt].pbw + (size_t)(f.base + lo) * f.dt, sx));
        return ROME_OK;
      });
      if (rc) return rc;
      rc = phase(nat, [&](int i, hipStream_t sx) -> int {
        const int t = typ_a[i];
        const rome_upsolve_plan::Type& y = P->type[t];
        const int pa = X.up_cnt_before[3 * (size_t)k0 + t], pb = X.up_cnt_before[3 * (size_t)k1 + t];
        // the product writes the new beliefs IN PLACE into the store (a product reads only proposals and its own variable's block)
        GibbsPlace place{y.block + pa, X.has_upstream ? y.stream + pa : nullptr, (X.has_mirror && mirror_out) ? y.mirror + pa : nullptr,
                               mirror_out, mirror_stride};
        ROME_HIP(c, launch_product_gibbs(kVdim[t], pb - pa, N, y.prop_rows, y.ptr + pa, y.rows, y.prop, y.pbw,
                                               st->bel[t], st->bel[t], (unsigned char*)trees + y.tree_off, kCircProd[t], P->pi, y.max_k,
                                               o->seed, base + kProdOff[t] + (X.has_upstream ? 0ull : (uint64_t)pa), sx, &place));
        return ROME_OK;
      });
      if (rc) return rc;
    }
  }
  if (!on_main) {   // the one join: everything after the run is ordered after it on the context's stream
    for (int e = 0; e < n_cur; ++e) ROME_HIP(c, hipStreamWaitEvent(s, ev_cur[e], 0));
    on_main = true;
  }
  if (X.has_mirror && P->gi > 0) {
    // updated variables whose product never ran (no proposals at all) still owe their block to the mirror: the product kernel handles
    // K = 0 (copy), so nothing to do here as long as the type has proposal rows; a type without any row keeps its beliefs
    for (int t = 0; t < 3; ++t) {
      const rome_upsolve_plan::Type& y = P->type[t];
      if (y.n_up && y.prop_rows == 0) {
        GibbsPlace place{y.block, nullptr, y.mirror, mirror_out, mirror_stride};
        ROME_HIP(c, launch_product_gibbs(kVdim[t], y.n_up, N, 0, y.ptr, y.rows, y.prop, y.pbw, st->bel[t], st->bel[t],
                                               (unsigned char*)trees + y.tree_off, kCircProd[t], 1, 1, o->seed, 0, s, &place));
      }
    }
  }
  // ---- results (only when the plan was created with host outputs): the updated beliefs and their manikde! bandwidths
  bool sync = false;
  for (int t = 0; t < 3; ++t) {
    const rome_upsolve_plan::Type& y = P->type[t];
    const int nu = y.n_up;
    if (nu == 0) continue;
    if (y.bw_host) {
      ROME_HIP(c, launch_kde_bandwidth(kVdim[t], nu, N, st->bel[t], kCircBw[t], 1e-2, 1e-6, y.bwout, s, y.block));
      ROME_HIP(c, hipMemcpyAsync(y.bw_host, y.bwout, (size_t)nu * kVdim[t] * 8, hipMemcpyDeviceToHost, s));
      sync = true;
    }
    if (y.new_host) {
      ROME_HIP(c, launch_scatter_blocks(nu, N, y.gather, y.newout, (int64_t)kVdim[t] * N, st->bel[0], st->bel[1], st->bel[2], s, /*to_store=*/0));
      if ((rc = fetch_blocks(c, P->layout, nu, kVdim[t], N, y.newout, y.new_host))) return rc;
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
  const double* const vhost[3] = {q->bel_pose2, q->bel_point2, q->bel_pose3};
  for (int t = 0; t < 3; ++t) if (nv[t] < 0 || (nv[t] > 0 && !vhost[t])) return ROME_ERR_INVALID_ARG;
  if (u->up_mirror) return ROME_ERR_INVALID_ARG;   // (mirrors belong to plans: there is no device buffer to mirror into here)
  for (int k = 0; k < u->n_up; ++k) {               // the results are read back: every updated type needs its host outputs
    const int t = u->up_type ? u->up_type[k] : -1;
    if (t < 0 || t > 2) return ROME_ERR_INVALID_ARG;
    double* nh[3] = {u->new_pose2, u->new_point2, u->new_pose3}; double* bh[3] = {u->bw_pose2, u->bw_point2, u->bw_pose3};
    if (!nh[t] || !bh[t]) return ROME_ERR_INVALID_ARG;
  }
  ROME_BIND(c);
  rome_store st;
  st.ctx = c; st.N = N;
  for (int t = 0; t < 3; ++t) st.nv[t] = nv[t];
  {
    DrainOnExit drain{c->stream};
    if ((rc = carve_ctx(c, 11, [&](ArenaCursor& a) { lay_beliefs(a, nv, N, st.bel); return (int)ROME_OK; }))) return rc;
    if ((rc = stage_beliefs(c, o->layout, nv, N, vhost, st.bel))) return rc;
  }
  rome_upsolve_plan P;
  if ((rc = plan_build(c, &st, o, u, &P, true))) return rc;
  return plan_run(&P, o, nullptr, 0);
}

}  // extern "C"
