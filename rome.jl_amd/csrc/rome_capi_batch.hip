// rome_capi_batch.hip -- parametric linearisation, belief statistics, KDE, products and raw device memory behind the extern "C"
// boundary of librome_mi355.so.  Host-side plumbing only: argument checks, staging through the context's workspaces, launches.
#include "rome_capi_internal.h"

using namespace rome;

extern "C" {

/* ---- parametric linearisation ---- */
static bool lin_dims_host(int kind, int& dz, int& dr, int& da, int& db) {
  switch (kind) {
    case ROME_FACTOR_PRIORPOSE2: dz = 3; dr = 3; da = 3; db = 0; return true;
    case ROME_FACTOR_POSE2POSE2: dz = 3; dr = 3; da = 3; db = 3; return true;
    case ROME_FACTOR_POSE2POINT2BR: dz = 2; dr = 2; da = 3; db = 2; return true;
    case ROME_FACTOR_PRIORPOINT2: dz = 2; dr = 2; da = 2; db = 0; return true;
    case ROME_FACTOR_POSE3POSE3: dz = 6; dr = 6; da = 6; db = 6; return true;
    case ROME_FACTOR_PRIORPOSE3: dz = 6; dr = 6; da = 6; db = 0; return true;
    case ROME_FACTOR_POSE2POINT2BEARING: dz = 1; dr = 1; da = 3; db = 2; return true;
    default: return false;
  }
}
int rome_linearize_dev(rome_ctx* c, int32_t kind, int32_t F, const double* mu, const double* W, const double* xa,
                       const double* xb, double* r, double* Ja, double* Jb) {
  int dz, dr, da, db;
  if (!c || F < 0 || !lin_dims_host(kind, dz, dr, da, db)) return ROME_ERR_INVALID_ARG;
  // the device-pointer entry serves kinds 0..5: its one caller is the row-sharded multi-rank linearisation, which refuses
  // bearing-only factors by name (the host-pointer entry below serves kind 6)
  if (kind == ROME_FACTOR_POSE2POINT2BEARING) return ROME_ERR_INVALID_ARG;
  ROME_BIND(c);
  if (F > 0 && (!mu || !W || !xa || !r || !Ja || (db > 0 && (!xb || !Jb)))) return ROME_ERR_INVALID_ARG;
  ROME_HIP(c, launch_linearize(kind, F, mu, W, xa, xb, r, Ja, Jb, c->stream));
  return ROME_OK;
}
int rome_linearize(rome_ctx* c, int32_t kind, int32_t F, const double* mu, const double* W, const double* xa,
                   const double* xb, double* r, double* Ja, double* Jb) {
  int dz, dr, da, db;
  if (!c || F < 0 || !lin_dims_host(kind, dz, dr, da, db)) return ROME_ERR_INVALID_ARG;
  if (F == 0) return ROME_OK;
  if (!mu || !W || !xa || !r || !Ja || (db > 0 && (!xb || !Jb))) return ROME_ERR_INVALID_ARG;
  ROME_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  void *d_mu, *d_W, *d_xa, *d_xb = nullptr, *d_r, *d_Ja, *d_Jb = nullptr;
  int rc;
  const size_t n = (size_t)F;
  if ((rc = ensure(c, 0, 8 * n * dz, &d_mu))) return rc;
  if ((rc = ensure(c, 1, 8 * n * dr * dr, &d_W))) return rc;
  if ((rc = ensure(c, 2, 8 * n * da, &d_xa))) return rc;
  if ((rc = ensure(c, 4, 8 * n * dr, &d_r))) return rc;
  if ((rc = ensure(c, 5, 8 * n * dr * da, &d_Ja))) return rc;
  ROME_HIP(c, hipMemcpyAsync(d_mu, mu, 8 * n * dz, hipMemcpyHostToDevice, s));
  ROME_HIP(c, hipMemcpyAsync(d_W, W, 8 * n * dr * dr, hipMemcpyHostToDevice, s));
  ROME_HIP(c, hipMemcpyAsync(d_xa, xa, 8 * n * da, hipMemcpyHostToDevice, s));
  if (db > 0) {
    if ((rc = ensure(c, 3, 8 * n * db, &d_xb))) return rc;
    if ((rc = ensure(c, 6, 8 * n * dr * db, &d_Jb))) return rc;
    ROME_HIP(c, hipMemcpyAsync(d_xb, xb, 8 * n * db, hipMemcpyHostToDevice, s));
  }
  ROME_HIP(c, launch_linearize(kind, F, (const double*)d_mu, (const double*)d_W, (const double*)d_xa,
                                     (const double*)d_xb, (double*)d_r, (double*)d_Ja, (double*)d_Jb, s));
  ROME_HIP(c, hipMemcpyAsync(r, d_r, 8 * n * dr, hipMemcpyDeviceToHost, s));
  ROME_HIP(c, hipMemcpyAsync(Ja, d_Ja, 8 * n * dr * da, hipMemcpyDeviceToHost, s));
  if (db > 0) ROME_HIP(c, hipMemcpyAsync(Jb, d_Jb, 8 * n * dr * db, hipMemcpyDeviceToHost, s));
  ROME_HIP(c, hipStreamSynchronize(s));
  return ROME_OK;
}

/* ---- belief statistics / product ---- */
int rome_belief_stats_dev(rome_ctx* c, int32_t dim, int32_t V, int32_t N, const double* bel, double* mean, double* sd) {
  if (!c || V < 0 || N < 1 || (dim != 2 && dim != 3 && dim != 6) || (V > 0 && (!bel || !mean || !sd))) return ROME_ERR_INVALID_ARG;
  ROME_BIND(c);
  ROME_HIP(c, launch_belief_stats(dim, V, N, bel, mean, sd, c->stream));
  return ROME_OK;
}
int rome_belief_stats(rome_ctx* c, int32_t dim, int32_t V, int32_t N, const double* bel, double* mean, double* sd) {
  if (!c || V < 0 || N < 1 || (dim != 2 && dim != 3 && dim != 6) || (V > 0 && (!bel || !mean || !sd))) return ROME_ERR_INVALID_ARG;
  if (V == 0) return ROME_OK;
  ROME_HIP(c, hipSetDevice(c->device));
  void *d_b, *d_m, *d_s; int rc;
  const size_t nb = 8ull * V * dim * N, nm = 8ull * V * dim;
  if ((rc = ensure(c, 0, nb, &d_b))) return rc;
  if ((rc = ensure(c, 1, nm, &d_m))) return rc;
  if ((rc = ensure(c, 2, nm, &d_s))) return rc;
  ROME_HIP(c, hipMemcpyAsync(d_b, bel, nb, hipMemcpyHostToDevice, c->stream));
  ROME_HIP(c, launch_belief_stats(dim, V, N, (const double*)d_b, (double*)d_m, (double*)d_s, c->stream));
  ROME_HIP(c, hipMemcpyAsync(mean, d_m, nm, hipMemcpyDeviceToHost, c->stream));
  ROME_HIP(c, hipMemcpyAsync(sd, d_s, nm, hipMemcpyDeviceToHost, c->stream));
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  return ROME_OK;
}
/* ---- mmd ---- */
static int check_mmd(rome_ctx* c, int32_t dim, int32_t P, int32_t Na, const double* a, int32_t Nb, const double* b, const double* scale,
                     double sigma, const double* out) {
  if (!c || P < 0 || Na < 1 || Nb < 1 || (dim != 2 && dim != 3 && dim != 6)) return ROME_ERR_INVALID_ARG;
  if (!std::isfinite(sigma) || sigma < 0.0) return ROME_ERR_INVALID_ARG;
  if (scale) for (int k = 0; k < dim; ++k) if (!std::isfinite(scale[k]) || scale[k] < 0.0) return ROME_ERR_INVALID_ARG;
  if (P > 0 && (!a || !b || !out)) return ROME_ERR_INVALID_ARG;
  if (Na > ROME_MAX_PARTICLES_MMD || Nb > ROME_MAX_PARTICLES_MMD) return ROME_ERR_UNSUPPORTED_N;   /* both sets live in LDS */
  return ROME_OK;
}
int rome_mmd_dev(rome_ctx* c, int32_t dim, int32_t P, int32_t Na, const double* a, const int32_t* a_rows, int32_t Nb, const double* b,
                 const int32_t* b_rows, const double* scale, double sigma, double* out, double* sums) {
  int rc = check_mmd(c, dim, P, Na, a, Nb, b, scale, sigma, out); if (rc) return rc;
  if (P == 0) return ROME_OK;
  ROME_BIND(c);
  ROME_HIP(c, launch_mmd(dim, P, Na, a, a_rows, Nb, b, b_rows, scale, sigma, out, sums, c->stream));
  return ROME_OK;
}
// rows of a host row table inside [0, n_blocks); without a table pair p reads block p
static bool mmd_rows_ok(const int32_t* rows, int P, int n_blocks) {
  if (!rows) return P <= n_blocks;
  for (int p = 0; p < P; ++p) if (rows[p] < 0 || rows[p] >= n_blocks) return false;
  return true;
}
int rome_mmd(rome_ctx* c, int32_t layout, int32_t dim, int32_t P, int32_t Na, int32_t n_a_blocks, const double* a, const int32_t* a_rows,
             int32_t Nb, int32_t n_b_blocks, const double* b, const int32_t* b_rows, const double* scale, double sigma, double* out,
             double* sums) {
  int rc = check_mmd(c, dim, P, Na, a, Nb, b, scale, sigma, out); if (rc) return rc;
  if (layout != ROME_LAYOUT_SOA && layout != ROME_LAYOUT_AOS && layout != ROME_LAYOUT_AOS_POINTS) return ROME_ERR_INVALID_ARG;
  if (n_a_blocks < 0 || n_b_blocks < 0 || !mmd_rows_ok(a_rows, P, n_a_blocks) || !mmd_rows_ok(b_rows, P, n_b_blocks)) return ROME_ERR_INVALID_ARG;
  if (P == 0) return ROME_OK;
  ROME_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  void *d_a, *d_b, *d_o, *d_s = nullptr, *d_ar = nullptr, *d_br = nullptr;
  const size_t np = (size_t)P;
  if ((rc = ensure(c, 0, 8ull * n_a_blocks * dim * Na, &d_a))) return rc;
  if ((rc = ensure(c, 1, 8ull * n_b_blocks * dim * Nb, &d_b))) return rc;
  if ((rc = ensure(c, 2, 8 * np, &d_o))) return rc;
  if (sums && (rc = ensure(c, 3, 24 * np, &d_s))) return rc;
  if ((rc = stage_blocks(c, layout, n_a_blocks, dim, Na, a, (double*)d_a))) return rc;
  if ((rc = stage_blocks(c, layout, n_b_blocks, dim, Nb, b, (double*)d_b))) return rc;
  if (a_rows) {
    if ((rc = ensure(c, 4, 4 * np, &d_ar))) return rc;
    ROME_HIP(c, hipMemcpyAsync(d_ar, a_rows, 4 * np, hipMemcpyHostToDevice, s));
  }
  if (b_rows) {
    if ((rc = ensure(c, 5, 4 * np, &d_br))) return rc;
    ROME_HIP(c, hipMemcpyAsync(d_br, b_rows, 4 * np, hipMemcpyHostToDevice, s));
  }
  ROME_HIP(c, launch_mmd(dim, P, Na, (const double*)d_a, (const int32_t*)d_ar, Nb, (const double*)d_b, (const int32_t*)d_br, scale, sigma,
                         (double*)d_o, (double*)d_s, s));
  ROME_HIP(c, hipMemcpyAsync(out, d_o, 8 * np, hipMemcpyDeviceToHost, s));
  if (sums) ROME_HIP(c, hipMemcpyAsync(sums, d_s, 24 * np, hipMemcpyDeviceToHost, s));
  ROME_HIP(c, hipStreamSynchronize(s));
  return ROME_OK;
}
/* ---- kde_eval ---- */
static int check_kde_eval(rome_ctx* c, int32_t dim, int32_t P, int32_t N, const double* bel, const double* bw, int32_t Q, const double* queries,
                          int32_t leave_one_out, const double* out) {
  if (!c || P < 0 || Q < 0 || N < 1 || (dim != 2 && dim != 3 && dim != 6)) return ROME_ERR_INVALID_ARG;
  if (!queries && Q != N) return ROME_ERR_INVALID_ARG;                           /* self-evaluation: the queries are the N particles */
  if (leave_one_out && (queries || N < 2)) return ROME_ERR_INVALID_ARG;
  if (P > 0 && Q > 0 && (!bel || !bw || !out)) return ROME_ERR_INVALID_ARG;
  if ((int64_t)P * ((Q + 255) / 256) > INT32_MAX) return ROME_ERR_INVALID_ARG;   /* one block per (pair, 256 queries) on a 1-D grid */
  if (N > ROME_MAX_PARTICLES_KDE_EVAL) return ROME_ERR_UNSUPPORTED_N;            /* the belief lives in LDS */
  return ROME_OK;
}
int rome_kde_eval_dev(rome_ctx* c, int32_t dim, int32_t P, int32_t N, const double* bel, const int32_t* bel_rows, const double* bw, int32_t Q,
                      const double* queries, const int32_t* query_rows, int32_t leave_one_out, double* out) {
  int rc = check_kde_eval(c, dim, P, N, bel, bw, Q, queries, leave_one_out, out); if (rc) return rc;
  if (P == 0 || Q == 0) return ROME_OK;
  ROME_BIND(c);
  ROME_HIP(c, launch_kde_eval(dim, P, N, bel, bel_rows, bw, Q, queries, query_rows, leave_one_out, out, c->stream));
  return ROME_OK;
}
int rome_kde_eval(rome_ctx* c, int32_t layout, int32_t dim, int32_t P, int32_t N, int32_t n_bel_blocks, const double* bel,
                  const int32_t* bel_rows, const double* bw, int32_t Q, int32_t n_query_blocks, const double* queries,
                  const int32_t* query_rows, int32_t leave_one_out, double* out) {
  int rc = check_kde_eval(c, dim, P, N, bel, bw, Q, queries, leave_one_out, out); if (rc) return rc;
  if (layout != ROME_LAYOUT_SOA && layout != ROME_LAYOUT_AOS && layout != ROME_LAYOUT_AOS_POINTS) return ROME_ERR_INVALID_ARG;
  if (n_bel_blocks < 0 || n_query_blocks < 0 || !mmd_rows_ok(bel_rows, P, n_bel_blocks)) return ROME_ERR_INVALID_ARG;
  if (queries && !mmd_rows_ok(query_rows, P, n_query_blocks)) return ROME_ERR_INVALID_ARG;
  if (bw) for (size_t k = 0; k < (size_t)n_bel_blocks * dim; ++k) if (!std::isfinite(bw[k]) || !(bw[k] > 0.0)) return ROME_ERR_INVALID_ARG;
  if (P == 0 || Q == 0) return ROME_OK;
  ROME_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  void *d_b, *d_q = nullptr, *d_o, *d_h, *d_br = nullptr, *d_qr = nullptr;
  const size_t np = (size_t)P, nh = 8ull * n_bel_blocks * dim, no = 8 * np * Q;
  if ((rc = ensure(c, 0, 8ull * n_bel_blocks * dim * N, &d_b))) return rc;
  if (queries && (rc = ensure(c, 1, 8ull * n_query_blocks * dim * Q, &d_q))) return rc;
  if ((rc = ensure(c, 2, no, &d_o))) return rc;
  if ((rc = ensure(c, 3, nh, &d_h))) return rc;
  if ((rc = stage_blocks(c, layout, n_bel_blocks, dim, N, bel, (double*)d_b))) return rc;
  if (queries && (rc = stage_blocks(c, layout, n_query_blocks, dim, Q, queries, (double*)d_q))) return rc;
  ROME_HIP(c, hipMemcpyAsync(d_h, bw, nh, hipMemcpyHostToDevice, s));
  if (bel_rows) {
    if ((rc = ensure(c, 4, 4 * np, &d_br))) return rc;
    ROME_HIP(c, hipMemcpyAsync(d_br, bel_rows, 4 * np, hipMemcpyHostToDevice, s));
  }
  if (queries && query_rows) {
    if ((rc = ensure(c, 5, 4 * np, &d_qr))) return rc;
    ROME_HIP(c, hipMemcpyAsync(d_qr, query_rows, 4 * np, hipMemcpyHostToDevice, s));
  }
  ROME_HIP(c, launch_kde_eval(dim, P, N, (const double*)d_b, (const int32_t*)d_br, (const double*)d_h, Q, (const double*)d_q,
                              (const int32_t*)d_qr, leave_one_out, (double*)d_o, s));
  ROME_HIP(c, hipMemcpyAsync(out, d_o, no, hipMemcpyDeviceToHost, s));
  ROME_HIP(c, hipStreamSynchronize(s));
  return ROME_OK;
}

static int check_kde(rome_ctx* c, int32_t dim, int32_t V, int32_t N, const double* bel, const double* bw) {
  if (!c || V < 0 || N < 2 || N > ROME_MAX_PARTICLES_REGISTER || dim < 1 || dim > 6 || (V > 0 && (!bel || !bw))) return ROME_ERR_INVALID_ARG;
  return ROME_OK;
}
int rome_kde_bandwidth_dev(rome_ctx* c, int32_t dim, int32_t V, int32_t N, const double* bel, uint32_t circular_mask,
                           double tol_euclid, double tol_circular, double* bw) {
  int rc = check_kde(c, dim, V, N, bel, bw); if (rc) return rc;
  ROME_BIND(c);
  ROME_HIP(c, launch_kde_bandwidth(dim, V, N, bel, circular_mask, tol_euclid > 0 ? tol_euclid : 1e-2,
                                         tol_circular > 0 ? tol_circular : 1e-6, bw, c->stream));
  return ROME_OK;
}
int rome_kde_bandwidth(rome_ctx* c, int32_t dim, int32_t V, int32_t N, const double* bel, uint32_t circular_mask,
                       double tol_euclid, double tol_circular, double* bw) {
  int rc = check_kde(c, dim, V, N, bel, bw); if (rc) return rc;
  if (V == 0) return ROME_OK;
  ROME_HIP(c, hipSetDevice(c->device));
  void *d_b, *d_h;
  const size_t nb = 8ull * V * dim * N, nh = 8ull * V * dim;
  if ((rc = ensure(c, 0, nb, &d_b))) return rc;
  if ((rc = ensure(c, 1, nh, &d_h))) return rc;
  ROME_HIP(c, hipMemcpyAsync(d_b, bel, nb, hipMemcpyHostToDevice, c->stream));
  ROME_HIP(c, launch_kde_bandwidth(dim, V, N, (const double*)d_b, circular_mask, tol_euclid > 0 ? tol_euclid : 1e-2,
                                         tol_circular > 0 ? tol_circular : 1e-6, (double*)d_h, c->stream));
  ROME_HIP(c, hipMemcpyAsync(bw, d_h, nh, hipMemcpyDeviceToHost, c->stream));
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  return ROME_OK;
}
int rome_kde_max_dev(rome_ctx* c, int32_t dim, int32_t V, int32_t N, const double* bel, const double* bw, int32_t grid_points,
                     double* out) {
  int rc = check_kde(c, dim, V, N, bel, bw); if (rc) return rc;
  ROME_BIND(c);
  const int G = grid_points > 0 ? grid_points : 200;
  if (G < 2 || G > 256 || (V > 0 && !out)) return ROME_ERR_INVALID_ARG;
  ROME_HIP(c, launch_kde_max(dim, V, N, G, 0.1, bel, bw, out, c->stream));
  return ROME_OK;
}
int rome_kde_max(rome_ctx* c, int32_t dim, int32_t V, int32_t N, const double* bel, const double* bw, int32_t grid_points, double* out) {
  int rc = check_kde(c, dim, V, N, bel, bw); if (rc) return rc;
  const int G = grid_points > 0 ? grid_points : 200;
  if (G < 2 || G > 256 || (V > 0 && !out)) return ROME_ERR_INVALID_ARG;
  if (V == 0) return ROME_OK;
  ROME_HIP(c, hipSetDevice(c->device));
  void *d_b, *d_h, *d_o;
  const size_t nb = 8ull * V * dim * N, nh = 8ull * V * dim;
  if ((rc = ensure(c, 0, nb, &d_b))) return rc;
  if ((rc = ensure(c, 1, nh, &d_h))) return rc;
  if ((rc = ensure(c, 2, nh, &d_o))) return rc;
  ROME_HIP(c, hipMemcpyAsync(d_b, bel, nb, hipMemcpyHostToDevice, c->stream));
  ROME_HIP(c, hipMemcpyAsync(d_h, bw, nh, hipMemcpyHostToDevice, c->stream));
  ROME_HIP(c, launch_kde_max(dim, V, N, G, 0.1, (const double*)d_b, (const double*)d_h, (double*)d_o, c->stream));
  ROME_HIP(c, hipMemcpyAsync(out, d_o, nh, hipMemcpyDeviceToHost, c->stream));
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  return ROME_OK;
}
int rome_product_bw_dev(rome_ctx* c, const rome_opts* o, int32_t dim, int32_t V, const int32_t* prop_ptr, const int32_t* prop_rows,
                        const double* prop, const double* prop_bw, const double* bel_in, double* bel_out) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || V < 0 || (dim != 2 && dim != 3 && dim != 6)) return ROME_ERR_INVALID_ARG;
  ROME_BIND(c);
  if (V > 0 && (!prop_ptr || !bel_in || !bel_out)) return ROME_ERR_INVALID_ARG;
  const int N = o->n_particles;
  if (dim == 6 && N > 256) return ROME_ERR_UNSUPPORTED_N;   /* Pose3 product: points staged in LDS */
  const double c_n = std::pow(4.0 / ((dim + 2.0) * N), 1.0 / (dim + 4.0));
  ROME_HIP(c, launch_product(dim, V, N, prop_ptr, prop_rows, prop, prop_bw, bel_in, bel_out, c_n, o->seed, o->stream_offset, c->stream));
  return ROME_OK;
}
int rome_product_dev(rome_ctx* c, const rome_opts* o, int32_t dim, int32_t V, const int32_t* prop_ptr, const int32_t* prop_rows,
                     const double* prop, const double* bel_in, double* bel_out) {
  return rome_product_bw_dev(c, o, dim, V, prop_ptr, prop_rows, prop, nullptr, bel_in, bel_out);
}

int rome_product_gibbs_dev(rome_ctx* c, const rome_opts* o, int32_t dim, int32_t V, const int32_t* prop_ptr, const int32_t* prop_rows,
                           const double* prop, const double* prop_bw, int32_t n_prop_rows, const double* bel_in, double* bel_out,
                           uint32_t circular_mask, int32_t gibbs_iters, int32_t max_proposals) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || V < 0 || n_prop_rows < 0 || (dim != 2 && dim != 3 && dim != 6) || max_proposals < 1) return ROME_ERR_INVALID_ARG;
  if (V > 0 && (!prop_ptr || !prop_rows || !bel_in || !bel_out)) return ROME_ERR_INVALID_ARG;
  if (n_prop_rows > 0 && (!prop || !prop_bw)) return ROME_ERR_INVALID_ARG;
  if (o->n_particles > ROME_MAX_PARTICLES_GIBBS) return ROME_ERR_UNSUPPORTED_N;   /* lane = output sample: 128- or 256-thread blocks */
  ROME_BIND(c);
  void* trees = nullptr;   /* one ball tree per proposal row, context-owned workspace (grown on demand, kept) */
  rc = ensure(c, 10, gibbs_workspace_bytes(dim, n_prop_rows, V, o->n_particles), &trees); if (rc) return rc;
  ROME_HIP(c, launch_product_gibbs(dim, V, o->n_particles, n_prop_rows, prop_ptr, prop_rows, prop, prop_bw, bel_in, bel_out, trees,
                                         circular_mask, gibbs_iters, max_proposals, o->seed, o->stream_offset, c->stream));
  return ROME_OK;
}

/* ---- partial-aware product, stage 2 ---- */
static int check_product_partial(rome_ctx* c, const rome_opts* o, int32_t dim, int32_t V, int32_t T, const int32_t* task_var,
                                 const int32_t* task_coord, const int32_t* task_ptr, const int32_t* task_rows, const int32_t* task_joint,
                                 const double* prop, double* bel) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || V < 0 || T < 0 || (dim != 2 && dim != 3 && dim != 6)) return ROME_ERR_INVALID_ARG;
  if (T > 0 && (!task_var || !task_coord || !task_ptr || !task_rows || !task_joint || !prop || !bel)) return ROME_ERR_INVALID_ARG;
  if (o->n_particles > ROME_MAX_PARTICLES_PRODUCT) return ROME_ERR_UNSUPPORTED_N;   /* stage 2 is 1-D: 512 at every dim */
  return ROME_OK;
}
int rome_product_partial_dev(rome_ctx* c, const rome_opts* o, int32_t dim, int32_t V, int32_t T, const int32_t* task_var,
                             const int32_t* task_coord, const int32_t* task_ptr, const int32_t* task_rows, const int32_t* task_joint,
                             const double* prop, const double* prop_bw, const double* joint_bw, uint32_t circular_mask, double* bel) {
  int rc = check_product_partial(c, o, dim, V, T, task_var, task_coord, task_ptr, task_rows, task_joint, prop, bel); if (rc) return rc;
  if (T == 0) return ROME_OK;
  ROME_BIND(c);
  ROME_HIP(c, launch_product_partial(dim, T, o->n_particles, task_var, task_coord, task_ptr, task_rows, task_joint, prop, prop_bw, joint_bw,
                                     circular_mask, bel, o->seed, o->stream_offset, c->stream));
  return ROME_OK;
}
int rome_product_partial(rome_ctx* c, const rome_opts* o, int32_t dim, int32_t V, int32_t T, const int32_t* task_var,
                         const int32_t* task_coord, const int32_t* task_ptr, const int32_t* task_rows, const int32_t* task_joint,
                         const double* prop, const double* prop_bw, const double* joint_bw, uint32_t circular_mask, double* bel,
                         int32_t n_prop_rows) {
  int rc = check_product_partial(c, o, dim, V, T, task_var, task_coord, task_ptr, task_rows, task_joint, prop, bel); if (rc) return rc;
  if (n_prop_rows < 0 || (T > 0 && (V < 1 || n_prop_rows < 1))) return ROME_ERR_INVALID_ARG;
  if (T == 0) return ROME_OK;
  ROME_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int N = o->n_particles;
  const size_t nt = 4ull * T, nr = 4ull * (size_t)(task_ptr[T] > 0 ? task_ptr[T] : 0);
  void *d_prop, *d_bel, *d_pbw = nullptr, *d_jbw = nullptr, *d_var, *d_coord, *d_ptr, *d_rows, *d_joint;
  if ((rc = ensure(c, 0, 8ull * n_prop_rows * dim * N, &d_prop))) return rc;
  if ((rc = ensure(c, 1, 8ull * V * dim * N, &d_bel))) return rc;
  if ((rc = ensure(c, 4, nt, &d_var))) return rc;
  if ((rc = ensure(c, 5, nt, &d_coord))) return rc;
  if ((rc = ensure(c, 6, nt + 4, &d_ptr))) return rc;
  if ((rc = ensure(c, 7, nr, &d_rows))) return rc;
  if ((rc = ensure(c, 8, nt, &d_joint))) return rc;
  if ((rc = stage_blocks(c, o->layout, n_prop_rows, dim, N, prop, (double*)d_prop))) return rc;
  if ((rc = stage_blocks(c, o->layout, V, dim, N, bel, (double*)d_bel))) return rc;
  if (prop_bw) {
    if ((rc = ensure(c, 2, 8ull * n_prop_rows * dim, &d_pbw))) return rc;
    ROME_HIP(c, hipMemcpyAsync(d_pbw, prop_bw, 8ull * n_prop_rows * dim, hipMemcpyHostToDevice, s));
  }
  if (joint_bw) {
    if ((rc = ensure(c, 3, 8ull * V * dim, &d_jbw))) return rc;
    ROME_HIP(c, hipMemcpyAsync(d_jbw, joint_bw, 8ull * V * dim, hipMemcpyHostToDevice, s));
  }
  ROME_HIP(c, hipMemcpyAsync(d_var, task_var, nt, hipMemcpyHostToDevice, s));
  ROME_HIP(c, hipMemcpyAsync(d_coord, task_coord, nt, hipMemcpyHostToDevice, s));
  ROME_HIP(c, hipMemcpyAsync(d_ptr, task_ptr, nt + 4, hipMemcpyHostToDevice, s));
  if (nr) ROME_HIP(c, hipMemcpyAsync(d_rows, task_rows, nr, hipMemcpyHostToDevice, s));
  ROME_HIP(c, hipMemcpyAsync(d_joint, task_joint, nt, hipMemcpyHostToDevice, s));
  ROME_HIP(c, launch_product_partial(dim, T, N, (const int32_t*)d_var, (const int32_t*)d_coord, (const int32_t*)d_ptr, (const int32_t*)d_rows,
                                     (const int32_t*)d_joint, (const double*)d_prop, (const double*)d_pbw, (const double*)d_jbw,
                                     circular_mask, (double*)d_bel, o->seed, o->stream_offset, s));
  return fetch_blocks(c, o->layout, V, dim, N, (const double*)d_bel, bel);   // (synchronises)
}

/* ---- device memory helpers ---- */
int rome_dev_alloc(rome_ctx* c, uint64_t bytes, void** out) {
  if (!c || !out) return ROME_ERR_INVALID_ARG;
  ROME_HIP(c, hipSetDevice(c->device));
  ROME_HIP(c, hipMalloc(out, bytes ? bytes : 8));
  return ROME_OK;
}
int rome_dev_free(rome_ctx* c, void* p) {
  if (!c) return ROME_ERR_INVALID_ARG;
  ROME_BIND(c);
  DevBuf b; b.p = p;   // (adopted for the one release)
  ROME_HIP(c, b.release());
  return ROME_OK;
}
int rome_dev_upload(rome_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c || (bytes && (!dst || !src))) return ROME_ERR_INVALID_ARG;
  ROME_BIND(c);
  ROME_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  return ROME_OK;
}
int rome_dev_download(rome_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c || (bytes && (!dst || !src))) return ROME_ERR_INVALID_ARG;
  ROME_BIND(c);
  ROME_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  return ROME_OK;
}

}  // extern "C"
