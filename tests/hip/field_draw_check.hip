// Exhaustive check of box_muller_field (rome.jl_amd/csrc/rome_device_math.hpp), the Box-Muller pair of the Pose2 draw, against the general
// box_muller on the words the draw is defined by; tests/test_gpu_field_draw.py compiles this with hipcc, runs it and reads the counts.
// One launch, one thread per 21-bit field f (2^21 threads, every index below 2^21 by construction of the grid: no memory is indexed by it):
//   radius  box_muller((f << 11) | 0x400, A) against box_muller_field with f on top of a word whose low 11 bits are all set, for two
//           fixed angle words A (one per sign of the angle); counted when n0 or n1 differs in any bit
//   angle   the same with f as the ANGLE field, for two fixed radius fields
//   pair c  field_word_c: the word built from (hi, lo) carries the low 11 bits of hi and bits 10..1 of lo on top
//   root    sqrt32_field(h) against the shipped sqrt32_rn_normal(h) at h = box_muller_h((f << 11) | 0x400)
//   bare    h * v_rsq_f32(h) without the correction step against sqrt32_rn_normal(h) (shows that the root comparison can fail)
// A thread counts in registers and adds its non-zero counts with vector atomics at the end.
//   field_draw_check -> "field radius <fields> <mismatches>" / "field angle <fields> <mismatches>" / "field pairc <fields> <mismatches>" /
//                       "field root <fields> <mismatches>" / "field bare <mismatches>" / "field_draw_check done"
#include <cstdio>
#include <cstdlib>
#include "../../rome.jl_amd/csrc/rome_device_math.hpp"
using namespace rome;

constexpr uint32_t kFields = 1u << 21;

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ __forceinline__ int pair_differs(uint32_t fr, uint32_t fa) {   // fields fr (radius), fa (angle)
  double g0, g1, n0, n1;
  box_muller((fr << 11) | 0x400u, (fa << 11) | 0x400u, &g0, &g1);
  box_muller_field((fr << 11) | 0x7FFu, (fa << 11) | 0x7FFu, &n0, &n1);
  return (__double_as_longlong(g0) != __double_as_longlong(n0) || __double_as_longlong(g1) != __double_as_longlong(n1)) ? 1 : 0;
}

// c[0] radius mismatches, c[1] angle, c[2] pair c, c[3] root, c[4] bare, c[5] fields visited
__global__ void __launch_bounds__(256) k_check(unsigned long long* c) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= kFields) return;
  const uint32_t others[2] = {0x0ABCDEu, 0x1F4321u};   // bit 18 (the sign of the angle) clear / set, quadrant bits 01 / 11
  unsigned long long rad = 0, ang = 0, pc = 0, root = 0, bare = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) { rad += pair_differs(f, others[k]); ang += pair_differs(others[k], f); }
  // pair c: f = the low 11 bits of hi, then bits 10..1 of lo; every other bit of hi and lo set
  const uint32_t hi = 0xFFFFF800u | (f >> 10), lo = 0xFFFFF801u | ((f & 0x3FFu) << 1);
  pc += (field_word_c(hi, lo) >> 11) == f ? 0 : 1;
  const float h = box_muller_h((f << 11) | 0x400u);
  const float want = sqrt32_rn_normal(h);
  root += same_bits(sqrt32_field(h), want) ? 0 : 1;
  bare += same_bits(h * __builtin_amdgcn_rsqf(h), want) ? 0 : 1;
  if (rad) atomicAdd(&c[0], rad);
  if (ang) atomicAdd(&c[1], ang);
  if (pc) atomicAdd(&c[2], pc);
  if (root) atomicAdd(&c[3], root);
  if (bare) atomicAdd(&c[4], bare);
  atomicAdd(&c[5], 1ull);
}

int main() {
  unsigned long long* d;
  unsigned long long h[8];
  if (hipMalloc(&d, 64) != hipSuccess) return 5;
  if (hipMemset(d, 0, 64) != hipSuccess) return 5;
  hipLaunchKernelGGL(k_check, dim3(kFields / 256), dim3(256), 0, 0, d);
  if (hipGetLastError() != hipSuccess) return 6;
  if (hipMemcpy(h, d, 64, hipMemcpyDeviceToHost) != hipSuccess) return 7;
  printf("field radius %llu %llu\n", h[5], h[0]);
  printf("field angle %llu %llu\n", h[5], h[1]);
  printf("field pairc %llu %llu\n", h[5], h[2]);
  printf("field root %llu %llu\n", h[5], h[3]);
  printf("field bare %llu\n", h[4]);
  printf("field_draw_check done\n");
  (void)hipFree(d);
  return 0;
}
