// rome_capi_internal.h -- what the units behind the extern "C" boundary share (rome_capi.hip, rome_capi_clique.hip, rome_capi_batch.hip):
// the context, error / device-binding helpers, the context's workspaces, owned device memory and the one layout staging pair.
#pragma once
#include "../../include/rome_mi355.h"
#include "rome_kernels.h"
#include "rome_layout.h"
#include "rome_upsolve_index.h"   // (al256, the arena cursor)

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

struct rome_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipError_t last_hip = hipSuccess;
  // 9 clique arena, 10 Gibbs trees, 11 / 12 temporary store / plan of the one-shot up-solve, 13 / 14 native points <-> coordinates
  static constexpr int kBufs = 15;
  void* dbuf[kBufs] = {nullptr};
  size_t dcap[kBufs] = {0};
  // pinned host staging of the host-pointer entry points (layout conversion writes straight into DMA-able memory)
  static constexpr int kHostBufs = 4;   // 0 fixed, 1 target (+ alternative landmark blocks), 2 noise, 3 out
  void* hbuf[kHostBufs] = {nullptr};
  size_t hcap[kHostBufs] = {0};
  // fork / join inside an up-solve step (plan_run): independent launches of a step -- the row families' convolutions + bandwidths, then
  // the products of the variable types -- go to side streams and re-join `stream`; created on first use
  static constexpr int kSide = 5;
  hipStream_t side[kSide] = {nullptr};
  hipEvent_t ev_fork = nullptr, ev_side[kSide] = {nullptr}, ev_side2[kSide] = {nullptr};   // two event sets: the phases alternate
  hipEvent_t ev_order = nullptr;   // rome_ctx_set_stream: the new stream is ordered after everything queued on the previous one
};

namespace rome {

inline int hip_fail(rome_ctx* c, hipError_t e) {
  if (c) c->last_hip = e;
  return ROME_ERR_HIP;
}
#define ROME_HIP(ctx, expr)                                   \
  do {                                                        \
    hipError_t _e = (expr);                                   \
    if (_e != hipSuccess) return rome::hip_fail((ctx), _e);   \
  } while (0)

// Every entry point that launches or copies, and every destroy function, binds the thread to the context's device first (a context
// created for device k must work whatever the caller's current device is); one hipGetDevice when it already is current.
inline hipError_t bind_device(const rome_ctx* c) {
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur == c->device) return hipSuccess;
  return hipSetDevice(c->device);
}
#define ROME_BIND(ctx) ROME_HIP((ctx), rome::bind_device(ctx))

// one device allocation, freed with its owner (whose destroy function binds the device before `delete`); move-only
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  ~DevBuf() { (void)release(); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
  hipError_t release() { void* q = p; p = nullptr; return q ? hipFree(q) : hipSuccess; }
};

// host vectors feed / receive asynchronous copies: whatever way an entry returns (an error in the middle included), the stream is
// drained before those vectors are destroyed (declare the guard AFTER them)
struct DrainOnExit { hipStream_t s; ~DrainOnExit() { (void)hipStreamSynchronize(s); } };

// the context's workspaces (grown on demand, kept), side streams, pinned staging
int ensure(rome_ctx* c, int idx, size_t bytes, void** out);
int ensure_side(rome_ctx* c);
int ensure_host(rome_ctx* c, int idx, size_t bytes, double** out);
int check_opts(const rome_opts* o);
void fill_args(ConvArgs& a, const rome_opts* o);

// rows of native points -> rows of coordinates (and back) on the device; host pointers; synchronises
int convert_rows(rome_ctx* c, int dim, size_t n, const double* src, double* dst, bool to_coords);

// THE layout conversion: n blocks of N particles in the caller's layout ([n][dim][N] SoA, [n][N][dim] AoS, [n][N][point_len] native
// points) <-> SoA coordinates at `dev`.  Native points go through the device conversion kernels (rows in, rows out), the transposition
// is a host copy.  `stage`: host memory for the SoA image (n * dim * N doubles, e.g. pinned) that outlives the stream work; nullptr:
// SoA moves straight between `host` and `dev`, other layouts use a temporary that stage_blocks drains the stream for.
// stage_blocks is asynchronous otherwise (`host` / `stage` must stay until the stream is drained); fetch_blocks synchronises.
int stage_blocks(rome_ctx* c, int layout, int n, int dim, int N, const double* host, double* dev, double* stage = nullptr);
int fetch_blocks(rome_ctx* c, int layout, int n, int dim, int N, const double* dev, double* host, double* stage = nullptr);

}  // namespace rome
