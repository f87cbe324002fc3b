// rome_capi.hip -- extern "C" boundary of librome_mi355.so (see include/rome_mi355.h).
// Host-side plumbing only: argument checks, Cholesky of the measurement covariances, layout
// conversion + staging for the host-pointer entry points, kernel launches.  No CPU compute path.
#include "rome_capi_internal.h"

using namespace rome;

int rome::ensure(rome_ctx* c, int idx, size_t bytes, void** out) {
  if (bytes == 0) bytes = 8;
  if (c->dcap[idx] < bytes) {
    if (c->dbuf[idx]) { hipError_t e = hipFree(c->dbuf[idx]); if (e != hipSuccess) return hip_fail(c, e); c->dbuf[idx] = nullptr; c->dcap[idx] = 0; }
    size_t cap = bytes + bytes / 4;
    hipError_t e = hipMalloc(&c->dbuf[idx], cap);
    if (e != hipSuccess) return hip_fail(c, e);
    c->dcap[idx] = cap;
  }
  *out = c->dbuf[idx];
  return ROME_OK;
}

int rome::ensure_side(rome_ctx* c) {
  if (c->ev_fork) return ROME_OK;
  for (int i = 0; i < rome_ctx::kSide; ++i) {   // (a failure half way leaves what exists for the next attempt and for rome_ctx_destroy)
    if (!c->side[i]) ROME_HIP(c, hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
    if (!c->ev_side[i]) ROME_HIP(c, hipEventCreateWithFlags(&c->ev_side[i], hipEventDisableTiming));
    if (!c->ev_side2[i]) ROME_HIP(c, hipEventCreateWithFlags(&c->ev_side2[i], hipEventDisableTiming));
  }
  ROME_HIP(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  return ROME_OK;
}

int rome::ensure_host(rome_ctx* c, int idx, size_t bytes, double** out) {
  if (bytes == 0) bytes = 8;
  if (c->hcap[idx] < bytes) {
    if (c->hbuf[idx]) { hipError_t e = hipHostFree(c->hbuf[idx]); if (e != hipSuccess) return hip_fail(c, e); c->hbuf[idx] = nullptr; c->hcap[idx] = 0; }
    size_t cap = bytes + bytes / 4;
    hipError_t e = hipHostMalloc(&c->hbuf[idx], cap, hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(c, e);
    c->hcap[idx] = cap;
  }
  *out = (double*)c->hbuf[idx];
  return ROME_OK;
}

int rome::check_opts(const rome_opts* o) {
  if (!o) return ROME_ERR_INVALID_ARG;
  if (o->n_particles < 1) return ROME_ERR_INVALID_ARG;
  if (o->n_particles > ROME_MAX_PARTICLES) return ROME_ERR_UNSUPPORTED_N;
  if (o->solver < ROME_SOLVER_CLOSED_FORM || o->solver > ROME_SOLVER_GAUSS_NEWTON) return ROME_ERR_INVALID_ARG;
  if (o->max_iters < 1 || o->inflate_cycles < 0 || o->inflate_cycles > 255) return ROME_ERR_INVALID_ARG;
  if (!(o->tol >= 0.0) || !(o->inflation >= 0.0) || !(o->spread_nh >= 0.0)) return ROME_ERR_INVALID_ARG;
  if (!(o->nullhypo >= 0.0 && o->nullhypo <= 1.0)) return ROME_ERR_INVALID_ARG;
  if (o->layout != ROME_LAYOUT_SOA && o->layout != ROME_LAYOUT_AOS && o->layout != ROME_LAYOUT_AOS_POINTS) return ROME_ERR_INVALID_ARG;
  if (o->presampled != ROME_NOISE_STANDARD_NORMALS && o->presampled != ROME_NOISE_MEASUREMENTS) return ROME_ERR_INVALID_ARG;
  return ROME_OK;
}

void rome::fill_args(ConvArgs& a, const rome_opts* o) {
  std::memset(&a, 0, sizeof(a));
  a.N = o->n_particles;
  a.max_iters = o->max_iters;
  a.cycles = o->inflate_cycles;
  a.tol = o->tol;
  a.inflation = o->inflation;
  a.inv_n = 1.0 / (double)o->n_particles;
  a.inv_nm1 = o->n_particles > 1 ? 1.0 / (double)(o->n_particles - 1) : 1.0;
  a.seed = o->seed;
  a.stream_offset = o->stream_offset;
  a.spread_nh = o->spread_nh;
  a.noise_is_meas = o->presampled == ROME_NOISE_MEASUREMENTS;
}

// rows of native points -> rows of coordinates (and back) on the device; host pointers.  Workspaces 13 / 14 are its own: a staging
// call converts one array while the previous one is still being uploaded into the entry point's buffers.
int rome::convert_rows(rome_ctx* c, int dim, size_t n, const double* src, double* dst, bool to_coords) {
  if (n == 0) return ROME_OK;
  const int pl = point_len(dim);
  if (dim == 2) { std::memcpy(dst, src, sizeof(double) * n * 2); return ROME_OK; }
  ROME_HIP(c, hipSetDevice(c->device));
  void *d_in, *d_out; int rc;
  const size_t nin = sizeof(double) * n * (to_coords ? pl : dim), nout = sizeof(double) * n * (to_coords ? dim : pl);
  if ((rc = ensure(c, 13, nin, &d_in))) return rc;
  if ((rc = ensure(c, 14, nout, &d_out))) return rc;
  ROME_HIP(c, hipMemcpyAsync(d_in, src, nin, hipMemcpyHostToDevice, c->stream));
  ROME_HIP(c, to_coords ? launch_points_to_coords((int)n, dim, (const double*)d_in, (double*)d_out, c->stream)
                        : launch_coords_to_points((int)n, dim, (const double*)d_in, (double*)d_out, c->stream));
  ROME_HIP(c, hipMemcpyAsync(dst, d_out, nout, hipMemcpyDeviceToHost, c->stream));
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  return ROME_OK;
}

// the one layout conversion (rome_capi_internal.h).  The conversion kernels read and write ROWS of points / coordinates and there is
// no transposition on the device, so a native-point array makes one device round trip (convert_rows) around the host transposition.
int rome::stage_blocks(rome_ctx* c, int layout, int n, int dim, int N, const double* host, double* dev, double* stage) {
  const size_t cnt = (size_t)n * dim * N;
  if (cnt == 0) return ROME_OK;
  std::vector<double> aos, tmp;
  const double* src = host;
  if (layout == ROME_LAYOUT_AOS_POINTS) {
    layout = ROME_LAYOUT_AOS;
    if (dim != 2) {   // (a Point2 point IS its coordinates)
      aos.resize(cnt);
      int rc = convert_rows(c, dim, (size_t)n * N, host, aos.data(), true); if (rc) return rc;
      src = aos.data();
    }
  }
  if (!stage && layout != ROME_LAYOUT_SOA) { tmp.resize(cnt); stage = tmp.data(); }
  if (stage) { to_soa(src, n, N, dim, layout, stage); src = stage; }
  ROME_HIP(c, hipMemcpyAsync(dev, src, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (!tmp.empty()) ROME_HIP(c, hipStreamSynchronize(c->stream));   // tmp goes out of scope
  return ROME_OK;
}
int rome::fetch_blocks(rome_ctx* c, int layout, int n, int dim, int N, const double* dev, double* host, double* stage) {
  const size_t cnt = (size_t)n * dim * N;
  if (cnt == 0) return ROME_OK;
  std::vector<double> tmp;
  if (!stage && layout != ROME_LAYOUT_SOA) { tmp.resize(cnt); stage = tmp.data(); }
  ROME_HIP(c, hipMemcpyAsync(stage ? stage : host, dev, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  if (!stage) return ROME_OK;
  if (layout != ROME_LAYOUT_AOS_POINTS || dim == 2) { from_soa(stage, n, N, dim, layout == ROME_LAYOUT_SOA ? layout : ROME_LAYOUT_AOS, host); return ROME_OK; }
  std::vector<double> aos(cnt);
  from_soa(stage, n, N, dim, ROME_LAYOUT_AOS, aos.data());
  return convert_rows(c, dim, (size_t)n * N, aos.data(), host, false);
}

namespace {

void args_from_dev(ConvArgs& a, const rome_opts* o, const rome_conv_dev* t) {
  fill_args(a, o);
  a.n_conv = t->n_conv; a.dir_all = t->dir_all;
  a.factor = t->factor; a.dir = t->dir; a.fixed_var = t->fixed_var; a.target_var = t->target_var;
  a.mu = t->mu; a.L = t->L; a.bel_fixed = t->bel_fixed; a.bel_target = t->bel_target;
  a.noise = t->noise; a.out = t->out; a.status = t->status;
  a.rows4 = t->rows4;
  a.n_mirror = t->mirror_out ? (t->n_mirror < 0 ? 0 : t->n_mirror) : 0;   // (> 4 is rejected by dev_common)
  for (int m = 0; m < 4; ++m) a.mirror_row[m] = t->mirror_row[m];
  a.mirror_out = t->mirror_out;
  a.mirror_map = t->mirror_out ? t->mirror_map : nullptr;
  a.alt_var = t->hypo_w ? t->alt_var : nullptr;
  a.hypo_w = t->hypo_w;
  a.nullhypo = t->nullhypo;
}

int cholesky_one(int d, const double* cov, double* Lp) {
  double L[36];
  std::memset(L, 0, sizeof(L));
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = cov[i * d + j];
      for (int k = 0; k < j; ++k) s -= L[i * d + k] * L[j * d + k];
      if (i == j) { if (!(s > 0.0)) return ROME_ERR_NOT_POSDEF; L[i * d + i] = std::sqrt(s); }
      else L[i * d + j] = s / L[j * d + j];
    }
  int k = 0;
  for (int i = 0; i < d; ++i) for (int j = 0; j <= i; ++j) Lp[k++] = L[i * d + j];
  return ROME_OK;
}

// ---- the factor families behind the convolution entries: everything their entry points differ in, said once.  A new family is a row
// of kFamily, its exported functions (one call each, below) and its wrapper in api.py.
enum FactorKind { kP2P2, kBR, kP3P3, kPrior2, kPrior3, kPriorPt2, kP2R, kPPR, kPB, kP3XYY, kP3ZRP, kP3ROT };
enum NoiseForm {   // how the noise parameters arrive at a host-pointer entry, and what the device table L holds
  kCov,            // cov [C][dz][dz] -> [C][dz (dz + 1) / 2], the row-packed lower Cholesky factor
  kSigma,          // sigma [C][dz], passed through (sigma < 0 encodes Uniform(mu ± |sigma|); NaN is refused)
  kZrp             // PriorPose3ZRP: sigma_z [C], cov_rp [C][2][2] -> [C][4] = [σ_z | packed 2x2 Cholesky of the roll / pitch covariance]
};
enum DirForm {     // how the direction arrives
  kDirNone,        // the family has none
  kDirRowsAny,     // a nullable per-row column, values unchecked: a row may be ROME_DIR_PRIOR
  kDirRows01,      // a nullable per-row column of 0 / 1
  kDirScalar       // one direction, 0 or 1, for the whole call (dir_all)
};
typedef hipError_t (*ConvLaunch)(const ConvArgs&, int solver, hipStream_t);
struct Family {
  int dz;                // dimension of the measurement
  int d1, d2;            // ... of the factor's first and second variable: direction 0 fixes the first and solves the second, 1 swaps
                         // them; d1 == 0: a sampler, nothing is fixed
  NoiseForm noise;
  DirForm dir;
  bool mh;               // alt_var / hypo_w of a device table reach the kernel (false: the _dev entry refuses them)
  bool fixed_is_target;  // a prior row that reads the target belief: the table's fixed block IS the target block (not read by the kernel)
  ConvLaunch launch;
};
constexpr Family kFamily[] = {
    /* kP2P2     */ {3, 3, 3, kCov, kDirRowsAny, true, false, launch_conv_pose2pose2},
    /* kBR       */ {2, 3, 2, kSigma, kDirScalar, true, false, launch_conv_bearingrange},
    /* kP3P3     */ {6, 6, 6, kCov, kDirRowsAny, true, false, launch_conv_pose3pose3},
    /* kPrior2   */ {3, 0, 3, kCov, kDirNone, true, false, [](const ConvArgs& a, int, hipStream_t s) { return launch_sample_priorpose2(a, s); }},
    /* kPrior3   */ {6, 0, 6, kCov, kDirNone, true, false, [](const ConvArgs& a, int, hipStream_t s) { return launch_sample_priorpose3(a, s); }},
    /* kPriorPt2 */ {2, 0, 2, kCov, kDirNone, true, false, [](const ConvArgs& a, int, hipStream_t s) { return launch_sample_priorpoint2(a, s); }},
    /* kP2R      */ {1, 2, 2, kSigma, kDirRows01, false, false, launch_conv_point2point2range},   // (a Point2 point IS its coordinates)
    /* kPPR      */ {1, 3, 2, kSigma, kDirScalar, false, false, launch_conv_pose2point2range},
    /* kPB       */ {1, 3, 2, kSigma, kDirScalar, false, false, launch_conv_pose2point2bearing},
    /* kP3XYY    */ {3, 6, 6, kCov, kDirRows01, false, false, launch_conv_pose3pose3xyyaw},
    /* kP3ZRP    */ {3, 6, 6, kZrp, kDirNone, false, true, [](const ConvArgs& a, int, hipStream_t s) { return launch_conv_priorpose3zrp(a, s); }},
    /* kP3ROT    */ {3, 6, 6, kCov, kDirRows01, false, false, launch_conv_pose3pose3rotation},
};
static_assert(sizeof(kFamily) / sizeof(kFamily[0]) == kP3ROT + 1, "one row per FactorKind, in its order");

// noise parameters of C rows -> the table L [C][nL] (kSigma: `prm` itself, nothing is packed); NaN or not positive definite: refused
int pack_noise(const Family& f, int C, const double* prm, const double* prm2, std::vector<double>& L, const double** Ltab, int* nL) {
  int rc;
  switch (f.noise) {
    case kCov:
      *nL = f.dz * (f.dz + 1) / 2;
      L.resize((size_t)C * *nL);
      if ((rc = rome_cholesky_lower(f.dz, C, prm, L.data()))) return rc;
      break;
    case kSigma:
      *nL = f.dz;
      for (int i = 0; i < C * f.dz; ++i) if (prm[i] != prm[i]) return ROME_ERR_NOT_POSDEF;   // (sigma < 0 encodes Uniform(mu ± |sigma|))
      *Ltab = prm;
      return ROME_OK;
    case kZrp:
      *nL = 4;
      L.resize((size_t)C * 4);
      for (int i = 0; i < C; ++i) {
        if (!(prm[i] >= 0.0)) return ROME_ERR_NOT_POSDEF;
        L[4 * (size_t)i] = prm[i];
        if ((rc = rome_cholesky_lower(2, 1, prm2 + 4 * (size_t)i, L.data() + 4 * (size_t)i + 1))) return rc;
      }
      break;
  }
  *Ltab = L.data();
  return ROME_OK;
}

// THE host-pointer convolution: checks (in the order the header states) -> pack the noise parameters -> stage -> launch -> fetch.
// dir: the per-row column of a kDirRows* family (nullable); dir_all: the scalar of a kDirScalar family and of every multihypo call.
// prm / prm2: the noise parameters as f.noise says.  alt / hypo_w: the multihypo entries (mh), C blocks of the other candidate.
int host_conv(rome_ctx* ctx, const rome_opts* o, FactorKind kind, int C, const int32_t* dir, int dir_all, const double* mu,
              const double* prm, const double* prm2, const double* fixed, const double* noise, double* target_inout, int32_t* status,
              bool mh = false, const double* alt = nullptr, const double* hypo_w = nullptr) {
  const Family& f = kFamily[kind];
  const bool has_fixed = f.d1 != 0, one_dir = mh || f.dir == kDirScalar;
  if (f.fixed_is_target) fixed = target_inout;   // (staged once more)
  int rc = check_opts(o); if (rc) return rc;
  if (!ctx || C < 0 || (one_dir && dir_all != 0 && dir_all != 1)) return ROME_ERR_INVALID_ARG;
  if (C > 0 && (!mu || !prm || (f.noise == kZrp && !prm2) || (has_fixed && !fixed) || !target_inout || (mh && (!alt || !hypo_w)))) return ROME_ERR_INVALID_ARG;
  if (C == 0) return ROME_OK;
  if (f.dir == kDirRows01 && dir) for (int i = 0; i < C; ++i) if (dir[i] != 0 && dir[i] != 1) return ROME_ERR_INVALID_ARG;
  if (mh) for (int i = 0; i < C; ++i) if (!(hypo_w[i] >= 0.0 && hypo_w[i] <= 1.0)) return ROME_ERR_INVALID_ARG;
  // the host vectors that asynchronous copies read, then the guard that drains the stream before any return destroys them
  std::vector<double> L, h_nh;
  std::vector<int32_t> h_alt;
  const double* Ltab; int nL;
  if ((rc = pack_noise(f, C, prm, prm2, L, &Ltab, &nL))) return rc;
  ROME_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DrainOnExit drain{s};

  const int N = o->n_particles, dz = f.dz, df = dir_all == 1 ? f.d2 : f.d1, dt = dir_all == 1 ? f.d1 : f.d2;
  const int lz = o->layout == ROME_LAYOUT_AOS_POINTS ? ROME_LAYOUT_AOS : o->layout;   // noise rows are measurement coordinates, never points
  // multihypo: the alternative landmark blocks are appended behind the landmark-side array
  const size_t blk_f = (size_t)C * N * df, blk_t = (size_t)C * N * dt;
  const size_t n_fixed = has_fixed ? blk_f * ((mh && dir_all == 1) ? 2 : 1) : 0;
  const size_t n_target = has_fixed ? blk_t * ((mh && dir_all != 1) ? 2 : 1) : 0;
  const size_t n_noise = noise ? (size_t)C * N * dz : 0;
  double *h_fixed = nullptr, *h_target = nullptr, *h_noise = nullptr, *h_out = nullptr;
  void *d_mu, *d_L, *d_fixed = nullptr, *d_target = nullptr, *d_noise = nullptr, *d_out, *d_dir = nullptr, *d_status = nullptr;
  if ((rc = ensure(ctx, 0, sizeof(double) * C * dz, &d_mu))) return rc;
  if ((rc = ensure(ctx, 1, sizeof(double) * C * nL, &d_L))) return rc;
  if ((rc = ensure(ctx, 2, sizeof(double) * blk_t, &d_out))) return rc;
  if ((rc = ensure_host(ctx, 3, sizeof(double) * blk_t, &h_out))) return rc;
  ROME_HIP(ctx, hipMemcpyAsync(d_mu, mu, sizeof(double) * C * dz, hipMemcpyHostToDevice, s));
  ROME_HIP(ctx, hipMemcpyAsync(d_L, Ltab, sizeof(double) * C * nL, hipMemcpyHostToDevice, s));
  if (has_fixed) {
    if ((rc = ensure_host(ctx, 0, sizeof(double) * n_fixed, &h_fixed))) return rc;
    if ((rc = ensure_host(ctx, 1, sizeof(double) * n_target, &h_target))) return rc;
    if ((rc = ensure(ctx, 3, sizeof(double) * n_fixed, &d_fixed))) return rc;
    if ((rc = ensure(ctx, 4, sizeof(double) * n_target, &d_target))) return rc;
    if ((rc = stage_blocks(ctx, o->layout, C, df, N, fixed, (double*)d_fixed, h_fixed))) return rc;
    if ((rc = stage_blocks(ctx, o->layout, C, dt, N, target_inout, (double*)d_target, h_target))) return rc;
    if (mh) {
      rc = dir_all == 1 ? stage_blocks(ctx, o->layout, C, df, N, alt, (double*)d_fixed + blk_f, h_fixed + blk_f)
                        : stage_blocks(ctx, o->layout, C, dt, N, alt, (double*)d_target + blk_t, h_target + blk_t);
      if (rc) return rc;
      h_alt.resize(C);
      for (int c = 0; c < C; ++c) h_alt[c] = C + c;
    }
  }
  if (noise) {
    if ((rc = ensure_host(ctx, 2, sizeof(double) * n_noise, &h_noise))) return rc;
    if ((rc = ensure(ctx, 5, sizeof(double) * n_noise, &d_noise))) return rc;
    if ((rc = stage_blocks(ctx, lz, C, dz, N, noise, (double*)d_noise, h_noise))) return rc;
  }
  if (dir) {
    if ((rc = ensure(ctx, 6, sizeof(int32_t) * C, &d_dir))) return rc;
    ROME_HIP(ctx, hipMemcpyAsync(d_dir, dir, sizeof(int32_t) * C, hipMemcpyHostToDevice, s));
  }
  if (status) { if ((rc = ensure(ctx, 7, sizeof(int32_t) * (size_t)C * N, &d_status))) return rc; }

  void *d_alt = nullptr, *d_hw = nullptr;
  if (!h_alt.empty()) {
    if ((rc = ensure(ctx, 8, sizeof(int32_t) * C, &d_alt))) return rc;
    if ((rc = ensure(ctx, 9, sizeof(double) * C, &d_hw))) return rc;
    ROME_HIP(ctx, hipMemcpyAsync(d_alt, h_alt.data(), sizeof(int32_t) * C, hipMemcpyHostToDevice, s));
    ROME_HIP(ctx, hipMemcpyAsync(d_hw, hypo_w, sizeof(double) * C, hipMemcpyHostToDevice, s));
  }
  void* d_nh = nullptr;
  if (o->nullhypo > 0.0 && has_fixed) {
    h_nh.assign((size_t)C, o->nullhypo);
    if ((rc = ensure(ctx, 10, sizeof(double) * C, &d_nh))) return rc;
    ROME_HIP(ctx, hipMemcpyAsync(d_nh, h_nh.data(), sizeof(double) * C, hipMemcpyHostToDevice, s));
  }
  ConvArgs a;
  fill_args(a, o);
  a.nullhypo = (const double*)d_nh;
  a.alt_var = (const int32_t*)d_alt; a.hypo_w = (const double*)d_hw;
  a.n_conv = C; a.dir_all = dir_all; a.dir = (const int32_t*)d_dir;
  a.mu = (const double*)d_mu; a.L = (const double*)d_L;
  a.bel_fixed = (const double*)d_fixed; a.bel_target = (const double*)d_target;
  a.noise = (const double*)d_noise; a.out = (double*)d_out; a.status = (int32_t*)d_status;
  ROME_HIP(ctx, f.launch(a, o->solver, s));
  if (status) ROME_HIP(ctx, hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t)C * N, hipMemcpyDeviceToHost, s));
  return fetch_blocks(ctx, o->layout, C, dt, N, (const double*)d_out, target_inout, h_out);   // (synchronises)
}

// rows of doubles: upload inputs, run, download
struct RowBuf { const double* host; int width; };
template <class Launch>
int host_rows(rome_ctx* ctx, int n, const RowBuf* in, int n_in, double* out, int out_width, Launch&& launch) {
  if (!ctx || n < 0 || !out) return ROME_ERR_INVALID_ARG;
  for (int k = 0; k < n_in; ++k) if (!in[k].host && n > 0) return ROME_ERR_INVALID_ARG;
  if (n == 0) return ROME_OK;
  ROME_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  void* d[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc;
  for (int k = 0; k < n_in; ++k) {
    if ((rc = ensure(ctx, k, sizeof(double) * (size_t)n * in[k].width, &d[k]))) return rc;
    ROME_HIP(ctx, hipMemcpyAsync(d[k], in[k].host, sizeof(double) * (size_t)n * in[k].width, hipMemcpyHostToDevice, s));
  }
  void* dout;
  if ((rc = ensure(ctx, 8, sizeof(double) * (size_t)n * out_width, &dout))) return rc;
  ROME_HIP(ctx, launch((const double*)d[0], (const double*)d[1], (const double*)d[2], (double*)dout, s));
  ROME_HIP(ctx, hipMemcpyAsync(out, dout, sizeof(double) * (size_t)n * out_width, hipMemcpyDeviceToHost, s));
  ROME_HIP(ctx, hipStreamSynchronize(s));
  return ROME_OK;
}

}  // namespace

extern "C" {

int rome_version(void) { return ROME_MI355_VERSION; }

const char* rome_strerror(int code) {
  switch (code) {
    case ROME_OK: return "ok";
    case ROME_ERR_INVALID_ARG: return "invalid argument";
    case ROME_ERR_NO_DEVICE: return "no HIP device available (librome_mi355 has no CPU fallback)";
    case ROME_ERR_HIP: return "HIP runtime error (see rome_last_hip_error_string)";
    case ROME_ERR_NOT_POSDEF: return "covariance is not positive definite";
    case ROME_ERR_UNSUPPORTED_N: return "n_particles exceeds ROME_MAX_PARTICLES";
    case ROME_ERR_ALLOC: return "host allocation failed";
    default: return "unknown error";
  }
}
int rome_last_hip_error(const rome_ctx* ctx) { return ctx ? (int)ctx->last_hip : 0; }
const char* rome_last_hip_error_string(const rome_ctx* ctx) { return hipGetErrorString(ctx ? ctx->last_hip : hipSuccess); }

void rome_opts_default(rome_opts* o, int32_t solver) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->n_particles = 100;
  o->solver = solver;
  o->max_iters = solver == ROME_SOLVER_NELDER_MEAD ? 1000 : 20;
  o->inflate_cycles = 3;
  o->tol = solver == ROME_SOLVER_NELDER_MEAD ? 1e-8 : 1e-12;
  o->inflation = 5.0;
  o->seed = 0x524F4D45ull; /* "ROME" */
  o->stream_offset = 0;
  o->layout = ROME_LAYOUT_SOA;
  o->spread_nh = 3.0;
}

int rome_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rome_ctx_create(rome_ctx** out, int device) {
  if (!out) return ROME_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ROME_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return ROME_ERR_INVALID_ARG;
  rome_ctx* c = new (std::nothrow) rome_ctx();
  if (!c) return ROME_ERR_ALLOC;
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return ROME_ERR_HIP; }
  c->stream = c->own_stream;
  *out = c;
  return ROME_OK;
}

void rome_ctx_destroy(rome_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (int i = 0; i < rome_ctx::kBufs; ++i) if (c->dbuf[i]) (void)hipFree(c->dbuf[i]);
  for (int i = 0; i < rome_ctx::kHostBufs; ++i) if (c->hbuf[i]) (void)hipHostFree(c->hbuf[i]);
  for (int i = 0; i < rome_ctx::kSide; ++i) {
    if (c->side[i]) { (void)hipStreamSynchronize(c->side[i]); (void)hipStreamDestroy(c->side[i]); }
    if (c->ev_side[i]) (void)hipEventDestroy(c->ev_side[i]);
    if (c->ev_side2[i]) (void)hipEventDestroy(c->ev_side2[i]);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_order) (void)hipEventDestroy(c->ev_order);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int rome_ctx_set_stream(rome_ctx* c, void* hip_stream) {
  if (!c) return ROME_ERR_INVALID_ARG;
  if (c->stream != (hipStream_t)hip_stream) {
    // Everything launched through a context is ONE logical sequence whatever stream it runs on: belief stores, plans' arenas, the
    // context's workspaces and caller tensors written by an earlier entry are read by later ones.  A stream change therefore orders
    // the new stream after ALL work queued on the previous one -- unconditionally, by an event (no host synchronisation, a few µs):
    // the previous stream may be the private non-blocking one, which nothing else ever joins (round 5's race: a block operation on
    // the private stream, then a plan run on the caller's stream reading its blocks).
    ROME_BIND(c);
    if (!c->ev_order) ROME_HIP(c, hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming));
    ROME_HIP(c, hipEventRecord(c->ev_order, c->stream));
    ROME_HIP(c, hipStreamWaitEvent((hipStream_t)hip_stream, c->ev_order, 0));
  }
  c->stream = (hipStream_t)hip_stream;  // NULL is HIP's default (null) stream, e.g. torch's default stream
  return ROME_OK;
}
int rome_ctx_use_own_stream(rome_ctx* c) {
  if (!c) return ROME_ERR_INVALID_ARG;
  return rome_ctx_set_stream(c, (void*)c->own_stream);
}
int rome_ctx_synchronize(rome_ctx* c) {
  if (!c) return ROME_ERR_INVALID_ARG;
  ROME_HIP(c, hipStreamSynchronize(c->stream));
  return ROME_OK;
}

int rome_cholesky_lower(int32_t d, int32_t n, const double* cov, double* L) {
  if (d < 1 || d > 6 || n < 0 || (n > 0 && (!cov || !L))) return ROME_ERR_INVALID_ARG;
  const int nL = d * (d + 1) / 2;
  for (int i = 0; i < n; ++i) {
    int rc = cholesky_one(d, cov + (size_t)i * d * d, L + (size_t)i * nL);
    if (rc) return rc;
  }
  return ROME_OK;
}

/* ---- residual entry points: widths of the rows of z, a, b (0: none) and r, the kernel's kind, whether pose rows are native points ---- */
struct ResidualEntry { int zw, aw, bw, rw, kind, pts; };
static int host_residual(rome_ctx* c, const ResidualEntry& e, int32_t n, const double* z, const double* a, const double* b, double* r) {
  const RowBuf in[3] = {{z, e.zw}, {a, e.aw}, {b, e.bw}};
  return host_rows(c, n, in, e.bw ? 3 : 2, r, e.rw, [&](const double* dz, const double* da, const double* db, double* dr, hipStream_t s) {
    return launch_residual(e.kind, e.pts, n, dz, da, db, dr, s); });
}
int rome_residual_pose2pose2(rome_ctx* c, int32_t n, const double* z, const double* p, const double* q, double* r) {
  return host_residual(c, {3, 3, 3, 3, kResPose2Pose2, 0}, n, z, p, q, r);
}
int rome_residual_priorpose2(rome_ctx* c, int32_t n, const double* m, const double* p, double* r) {
  return host_residual(c, {3, 3, 0, 3, kResPriorPose2, 0}, n, m, p, nullptr, r);
}
int rome_residual_pose2point2br(rome_ctx* c, int32_t n, const double* z, const double* p, const double* l, double* r) {
  return host_residual(c, {2, 3, 2, 2, kResBearingRange, 0}, n, z, p, l, r);
}
int rome_residual_pose2point2br_pt(rome_ctx* c, int32_t n, const double* z, const double* p, const double* l, double* r) {
  return host_residual(c, {2, 6, 2, 2, kResBearingRange, 1}, n, z, p, l, r);
}
int rome_residual_pose3pose3(rome_ctx* c, int32_t n, const double* z, const double* p, const double* q, double* r) {
  return host_residual(c, {6, 6, 6, 6, kResPose3Pose3, 0}, n, z, p, q, r);
}
int rome_residual_pose3pose3_pt(rome_ctx* c, int32_t n, const double* z, const double* p, const double* q, double* r) {
  return host_residual(c, {6, 12, 12, 6, kResPose3Pose3, 1}, n, z, p, q, r);
}
int rome_residual_pose3pose3xyyaw(rome_ctx* c, int32_t n, const double* z, const double* p, const double* q, double* r) {
  return host_residual(c, {3, 6, 6, 3, kResPose3Pose3XYYaw, 0}, n, z, p, q, r);
}
int rome_residual_pose3pose3xyyaw_pt(rome_ctx* c, int32_t n, const double* z, const double* p, const double* q, double* r) {
  return host_residual(c, {3, 12, 12, 3, kResPose3Pose3XYYaw, 1}, n, z, p, q, r);
}
int rome_residual_pose3pose3rotation(rome_ctx* c, int32_t n, const double* z, const double* p, const double* q, double* r) {
  return host_residual(c, {3, 6, 6, 3, kResPose3Pose3Rotation, 0}, n, z, p, q, r);
}
int rome_residual_pose3pose3rotation_pt(rome_ctx* c, int32_t n, const double* z, const double* p, const double* q, double* r) {
  return host_residual(c, {3, 12, 12, 3, kResPose3Pose3Rotation, 1}, n, z, p, q, r);
}
int rome_residual_priorpose3(rome_ctx* c, int32_t n, const double* m, const double* p, double* r) {
  return host_residual(c, {6, 6, 0, 6, kResPriorPose3, 0}, n, m, p, nullptr, r);
}
int rome_residual_point2point2range(rome_ctx* c, int32_t n, const double* z, const double* xi, const double* lm, double* r) {
  return host_residual(c, {1, 2, 2, 1, kResPoint2Point2Range, 0}, n, z, xi, lm, r);
}
int rome_residual_pose2point2range(rome_ctx* c, int32_t n, const double* z, const double* p, const double* lm, double* r) {
  return host_residual(c, {1, 3, 2, 1, kResPose2Point2Range, 0}, n, z, p, lm, r);
}
int rome_residual_pose2point2bearing(rome_ctx* c, int32_t n, const double* z, const double* p, const double* l, double* r) {
  return host_residual(c, {1, 3, 2, 1, kResBearing, 0}, n, z, p, l, r);
}
int rome_residual_pose2point2bearing_pt(rome_ctx* c, int32_t n, const double* z, const double* p, const double* l, double* r) {
  return host_residual(c, {1, 6, 2, 1, kResBearing, 1}, n, z, p, l, r);
}

/* ---- host-pointer convolutions: host_conv(kind, C, dir column, dir scalar, mu, noise parameters, fixed, noise, target, status) ---- */
int rome_conv_pose2pose2(rome_ctx* c, const rome_opts* o, int32_t C, const int32_t* dir, const double* mu, const double* cov,
                         const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kP2P2, C, dir, 0, mu, cov, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_pose2pose2_mh(rome_ctx* c, const rome_opts* o, int32_t C, int32_t dir, const double* mu, const double* cov,
                            const double* fixed, const double* alt, const double* hypo_w, const double* noise,
                            double* target_inout, int32_t* status) {
  return host_conv(c, o, kP2P2, C, nullptr, dir, mu, cov, nullptr, fixed, noise, target_inout, status, true, alt, hypo_w);
}
int rome_conv_pose2point2br(rome_ctx* c, const rome_opts* o, int32_t C, int32_t dir, const double* mu, const double* sigma,
                            const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kBR, C, nullptr, dir, mu, sigma, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_pose2point2br_mh(rome_ctx* c, const rome_opts* o, int32_t C, int32_t dir, const double* mu, const double* sigma,
                               const double* fixed, const double* alt, const double* hypo_w, const double* noise,
                               double* target_inout, int32_t* status) {
  return host_conv(c, o, kBR, C, nullptr, dir, mu, sigma, nullptr, fixed, noise, target_inout, status, true, alt, hypo_w);
}
int rome_conv_pose3pose3(rome_ctx* c, const rome_opts* o, int32_t C, const int32_t* dir, const double* mu, const double* cov,
                         const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kP3P3, C, dir, 0, mu, cov, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_point2point2range(rome_ctx* c, const rome_opts* o, int32_t C, const int32_t* dir, const double* mu, const double* sigma,
                                const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kP2R, C, dir, 0, mu, sigma, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_pose2point2range(rome_ctx* c, const rome_opts* o, int32_t C, int32_t dir, const double* mu, const double* sigma,
                               const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kPPR, C, nullptr, dir, mu, sigma, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_pose2point2bearing(rome_ctx* c, const rome_opts* o, int32_t C, int32_t dir, const double* mu, const double* sigma,
                                 const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kPB, C, nullptr, dir, mu, sigma, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_pose3pose3xyyaw(rome_ctx* c, const rome_opts* o, int32_t C, const int32_t* dir, const double* mu, const double* cov,
                              const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kP3XYY, C, dir, 0, mu, cov, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_pose3pose3rotation(rome_ctx* c, const rome_opts* o, int32_t C, const int32_t* dir, const double* mu, const double* cov,
                                const double* fixed, const double* noise, double* target_inout, int32_t* status) {
  return host_conv(c, o, kP3ROT, C, dir, 0, mu, cov, nullptr, fixed, noise, target_inout, status);
}
int rome_conv_priorpose3zrp(rome_ctx* c, const rome_opts* o, int32_t C, const double* mu, const double* sigma_z, const double* cov_rp,
                            const double* noise, double* target_inout) {
  return host_conv(c, o, kP3ZRP, C, nullptr, 0, mu, sigma_z, cov_rp, nullptr, noise, target_inout, nullptr);
}
int rome_sample_priorpose2(rome_ctx* c, const rome_opts* o, int32_t C, const double* mu, const double* cov, const double* noise, double* out) {
  return host_conv(c, o, kPrior2, C, nullptr, 0, mu, cov, nullptr, nullptr, noise, out, nullptr);
}
int rome_sample_priorpose3(rome_ctx* c, const rome_opts* o, int32_t C, const double* mu, const double* cov, const double* noise, double* out) {
  return host_conv(c, o, kPrior3, C, nullptr, 0, mu, cov, nullptr, nullptr, noise, out, nullptr);
}
int rome_sample_priorpoint2(rome_ctx* c, const rome_opts* o, int32_t C, const double* mu, const double* cov, const double* noise, double* out) {
  return host_conv(c, o, kPriorPt2, C, nullptr, 0, mu, cov, nullptr, nullptr, noise, out, nullptr);
}

/* ---- device-pointer convolutions ---- */
static int dev_common(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t, bool need_beliefs) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || !t || t->n_conv < 0) return ROME_ERR_INVALID_ARG;
  if (t->n_conv > 0 && (!t->mu || !t->L || !t->out)) return ROME_ERR_INVALID_ARG;
  if (t->n_conv > 0 && need_beliefs && (!t->bel_fixed || !t->bel_target)) return ROME_ERR_INVALID_ARG;
  if (t->mirror_out && !t->mirror_map && t->n_mirror > 4) return ROME_ERR_INVALID_ARG;   // mirror_row holds 4 rows (never silently dropped); more: mirror_map
  ROME_BIND(c);
  return ROME_OK;
}
// THE device-pointer convolution: the family's refusals (kFamily) -> common checks + device binding -> arguments -> launch on the
// context's stream
static int dev_conv(rome_ctx* c, const rome_opts* o, FactorKind kind, const rome_conv_dev* t) {
  const Family& f = kFamily[kind];
  if (t) {
    const bool dir01 = t->dir_all == 0 || t->dir_all == 1;
    if (!f.mh && (t->alt_var || t->hypo_w)) return ROME_ERR_INVALID_ARG;                          // no multihypo on this family
    if (f.dir == kDirScalar && (t->dir || !dir01)) return ROME_ERR_INVALID_ARG;                   // one direction per call
    if (f.dir == kDirRows01 && !t->dir && !t->rows4 && !dir01) return ROME_ERR_INVALID_ARG;       // a direction column, or 0 / 1 for all rows
  }
  int rc = dev_common(c, o, t, f.d1 != 0 && !f.fixed_is_target); if (rc) return rc;
  if (f.fixed_is_target && t->n_conv > 0 && !t->bel_target) return ROME_ERR_INVALID_ARG;   // the target belief is read: the proposal is its own particle, partly replaced
  ConvArgs a; args_from_dev(a, o, t);
  if (f.fixed_is_target) a.bel_fixed = a.bel_target;   // (fixed = target in every row; the block is not read)
  ROME_HIP(c, f.launch(a, o->solver, c->stream));
  return ROME_OK;
}
int rome_conv_pose2pose2_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kP2P2, t); }
int rome_conv_pose2point2br_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kBR, t); }
int rome_conv_point2point2range_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kP2R, t); }
int rome_conv_pose2point2range_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kPPR, t); }
int rome_conv_pose2point2bearing_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kPB, t); }
int rome_conv_pose3pose3_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kP3P3, t); }
int rome_conv_pose3pose3xyyaw_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kP3XYY, t); }
int rome_conv_pose3pose3rotation_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kP3ROT, t); }
int rome_conv_priorpose3zrp_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kP3ZRP, t); }
int rome_sample_priorpose2_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kPrior2, t); }
int rome_sample_priorpose3_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kPrior3, t); }
int rome_sample_priorpoint2_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* t) { return dev_conv(c, o, kPriorPt2, t); }
int rome_sweep_pose2_dev(rome_ctx* c, const rome_opts* o, const rome_conv_dev* p2p2, const rome_conv_dev* br1, const rome_conv_dev* br0,
                         const uint64_t* family_stream_offset) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || (!p2p2 && !br1 && !br0)) return ROME_ERR_INVALID_ARG;
  const rome_conv_dev* t[3] = {p2p2, br1, br0};
  ConvArgs a[3];
  for (int k = 0; k < 3; ++k) {
    if (!t[k]) continue;
    if ((rc = dev_common(c, o, t[k], true))) return rc;
    if (k > 0 && (t[k]->dir != nullptr || t[k]->dir_all != (k == 1 ? 1 : 0))) return ROME_ERR_INVALID_ARG;
    rome_opts of = *o;
    if (family_stream_offset) of.stream_offset = o->stream_offset + family_stream_offset[k];
    args_from_dev(a[k], &of, t[k]);
  }
  ROME_HIP(c, launch_sweep_pose2(p2p2 ? &a[0] : nullptr, br1 ? &a[1] : nullptr, br0 ? &a[2] : nullptr, o->solver, c->stream));
  return ROME_OK;
}

/* ---- approxDeconv: ROME_DECONV_* -> the convolution family whose table formats it shares, the unit that owns its policy ---- */
typedef hipError_t (*DeconvLaunch)(int, const DeconvArgs&, hipStream_t);
struct DeconvFamily { FactorKind kind; int kfam; DeconvLaunch launch; };
static const DeconvFamily kDeconv[] = {
    /* ROME_DECONV_POSE2POSE2         */ {kP2P2, kDeconvPose2Pose2, launch_deconv_pose2},
    /* ROME_DECONV_POSE2POINT2BR      */ {kBR, kDeconvBearingRange, launch_deconv_pose2},
    /* ROME_DECONV_POSE2POINT2BEARING */ {kPB, kDeconvBearing, launch_deconv_range},
    /* ROME_DECONV_POINT2POINT2RANGE  */ {kP2R, kDeconvPoint2Point2Range, launch_deconv_range},
    /* ROME_DECONV_POSE2POINT2RANGE   */ {kPPR, kDeconvPose2Point2Range, launch_deconv_range},
    /* ROME_DECONV_POSE3POSE3         */ {kP3P3, kDeconvPose3Pose3, launch_deconv_pose3},
    /* ROME_DECONV_POSE3POSE3XYYAW    */ {kP3XYY, kDeconvPose3Pose3XYYaw, launch_deconv_pose3_partial},
    /* ROME_DECONV_POSE3POSE3ROTATION */ {kP3ROT, kDeconvPose3Pose3Rotation, launch_deconv_pose3_partial},
};
static_assert(sizeof(kDeconv) / sizeof(kDeconv[0]) == ROME_DECONV_POSE3POSE3ROTATION + 1, "one row per ROME_DECONV_*, in its order");
static bool deconv_family_ok(int32_t family) { return family >= 0 && family <= ROME_DECONV_POSE3POSE3ROTATION; }
static void deconv_args(DeconvArgs& a, const rome_opts* o, const rome_deconv_table* t) {
  std::memset(&a, 0, sizeof(a));
  a.n_rows = t->n_rows; a.N = o->n_particles;
  a.rows4 = t->rows4; a.factor = t->factor; a.var_a = t->var_a; a.var_b = t->var_b;
  a.mu = t->mu; a.L = t->L; a.bel_a = t->bel_a; a.bel_b = t->bel_b; a.noise = t->noise;
  a.noise_is_meas = o->presampled == ROME_NOISE_MEASUREMENTS;
  a.pred = t->pred; a.meas = t->meas;
  a.seed = o->seed; a.stream_offset = o->stream_offset;
}
int rome_deconv_dev(rome_ctx* c, const rome_opts* o, int32_t family, const rome_deconv_table* t) {
  int rc = check_opts(o); if (rc) return rc;
  if (!c || !t || t->n_rows < 0 || !deconv_family_ok(family)) return ROME_ERR_INVALID_ARG;
  if (t->n_rows > 0 && (!t->mu || !t->L || !t->bel_a || !t->bel_b || (!t->pred && !t->meas))) return ROME_ERR_INVALID_ARG;
  if (t->n_rows == 0) return ROME_OK;
  ROME_BIND(c);
  DeconvArgs a; deconv_args(a, o, t);
  ROME_HIP(c, kDeconv[family].launch(kDeconv[family].kfam, a, c->stream));
  return ROME_OK;
}
int rome_deconv(rome_ctx* ctx, const rome_opts* o, int32_t family, int32_t C, const double* mu, const double* cov, const double* a,
                const double* b, const double* noise, double* pred, double* meas) {
  int rc = check_opts(o); if (rc) return rc;
  if (!ctx || C < 0 || !deconv_family_ok(family)) return ROME_ERR_INVALID_ARG;
  if (C > 0 && (!mu || !cov || !a || !b || (!pred && !meas))) return ROME_ERR_INVALID_ARG;
  if (C == 0) return ROME_OK;
  const Family& f = kFamily[kDeconv[family].kind];
  std::vector<double> L;
  const double* Ltab; int nL;
  if ((rc = pack_noise(f, C, cov, nullptr, L, &Ltab, &nL))) return rc;
  ROME_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DrainOnExit drain{s};
  const int N = o->n_particles, dz = f.dz;
  const int lz = o->layout == ROME_LAYOUT_AOS_POINTS ? ROME_LAYOUT_AOS : o->layout;   // measurement rows are coordinates, never points
  const size_t n_a = (size_t)C * N * f.d1, n_b = (size_t)C * N * f.d2, n_z = (size_t)C * N * dz;
  double *h_a, *h_b, *h_noise = nullptr, *h_out;
  void *d_mu, *d_L, *d_a, *d_b, *d_noise = nullptr, *d_pred = nullptr, *d_meas = nullptr;
  if ((rc = ensure(ctx, 0, sizeof(double) * C * dz, &d_mu))) return rc;
  if ((rc = ensure(ctx, 1, sizeof(double) * C * nL, &d_L))) return rc;
  if ((rc = ensure(ctx, 3, sizeof(double) * n_a, &d_a))) return rc;
  if ((rc = ensure(ctx, 4, sizeof(double) * n_b, &d_b))) return rc;
  if ((rc = ensure_host(ctx, 0, sizeof(double) * n_a, &h_a))) return rc;
  if ((rc = ensure_host(ctx, 1, sizeof(double) * n_b, &h_b))) return rc;
  if ((rc = ensure_host(ctx, 3, sizeof(double) * n_z, &h_out))) return rc;
  if (pred && (rc = ensure(ctx, 2, sizeof(double) * n_z, &d_pred))) return rc;
  if (meas && (rc = ensure(ctx, 6, sizeof(double) * n_z, &d_meas))) return rc;
  ROME_HIP(ctx, hipMemcpyAsync(d_mu, mu, sizeof(double) * C * dz, hipMemcpyHostToDevice, s));
  ROME_HIP(ctx, hipMemcpyAsync(d_L, Ltab, sizeof(double) * C * nL, hipMemcpyHostToDevice, s));
  if ((rc = stage_blocks(ctx, o->layout, C, f.d1, N, a, (double*)d_a, h_a))) return rc;
  if ((rc = stage_blocks(ctx, o->layout, C, f.d2, N, b, (double*)d_b, h_b))) return rc;
  if (noise) {
    if ((rc = ensure_host(ctx, 2, sizeof(double) * n_z, &h_noise))) return rc;
    if ((rc = ensure(ctx, 5, sizeof(double) * n_z, &d_noise))) return rc;
    if ((rc = stage_blocks(ctx, lz, C, dz, N, noise, (double*)d_noise, h_noise))) return rc;
  }
  rome_deconv_table t;
  std::memset(&t, 0, sizeof(t));
  t.n_rows = C; t.mu = (const double*)d_mu; t.L = (const double*)d_L; t.bel_a = (const double*)d_a; t.bel_b = (const double*)d_b;
  t.noise = (const double*)d_noise; t.pred = (double*)d_pred; t.meas = (double*)d_meas;
  DeconvArgs da; deconv_args(da, o, &t);
  ROME_HIP(ctx, kDeconv[family].launch(kDeconv[family].kfam, da, s));
  if (pred && (rc = fetch_blocks(ctx, lz, C, dz, N, (const double*)d_pred, pred, h_out))) return rc;   // (synchronises)
  if (meas && (rc = fetch_blocks(ctx, lz, C, dz, N, (const double*)d_meas, meas, h_out))) return rc;
  return ROME_OK;
}

/* ---- native point containers <-> coordinates ---- */
int rome_points_to_coords(rome_ctx* c, int32_t dim, int32_t n, const double* pts, double* coords) {
  if (!c || n < 0 || (dim != 2 && dim != 3 && dim != 6) || (n > 0 && (!pts || !coords))) return ROME_ERR_INVALID_ARG;
  return convert_rows(c, dim, (size_t)n, pts, coords, true);
}
int rome_coords_to_points(rome_ctx* c, int32_t dim, int32_t n, const double* coords, double* pts) {
  if (!c || n < 0 || (dim != 2 && dim != 3 && dim != 6) || (n > 0 && (!pts || !coords))) return ROME_ERR_INVALID_ARG;
  return convert_rows(c, dim, (size_t)n, coords, pts, false);
}

}  // extern "C"
