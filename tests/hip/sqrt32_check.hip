// Exhaustive check of sqrt32_rn_normal (rome.jl_amd/csrc/rome_device_math.hpp) against the compiler's correctly rounded expansion of
// __builtin_sqrtf; tests/test_gpu_sqrt32.py compiles this with hipcc, runs it and reads the counts.
//   pass 1: every float from bit pattern 0x0F800000 (2^-96) to 0x7F7FFFFF (the largest finite one): the documented range
//   pass 2: all 2^32 radius words wa through box_muller_h: wherever box_muller takes the root (h > 0), the same equality at that h;
//           such an h below 2^-96 is counted as out of range
// One grid-stride kernel; a thread counts in registers and adds its non-zero counts with vector atomics at the end.
//   sqrt32_check   -> prints "sqrt32 range <compared> <mismatches>" / "sqrt32 radius <h > 0> <mismatches> <out of range>" /
//                     "sqrt32 estimate <mismatches of the bare hardware estimate on pass 1>" (shows that the comparison can fail) / "sqrt32_check done"
#include <cstdio>
#include <cstdlib>
#include "../../rome.jl_amd/csrc/rome_device_math.hpp"
using namespace rome;

constexpr uint32_t kLo = 0x0F800000u, kHi = 0x7F7FFFFFu;

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// c[0] compared, c[1] mismatches, c[2] out of range (pass 2), c[3] mismatches of the bare estimate
template <int PASS>
__global__ void __launch_bounds__(256) k_check(unsigned long long first, unsigned long long count, unsigned long long* c) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long n = 0, bad = 0, out = 0, raw = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const uint32_t w = (uint32_t)(first + i);
    float x;
    if (PASS == 1) x = __uint_as_float(w);
    else {
      x = box_muller_h(w);
      if (!(x > 0.0f)) continue;                       // box_muller's select: no root taken
      if (x < __uint_as_float(kLo)) { ++out; continue; }
    }
    const float want = __builtin_sqrtf(x);
    ++n;
    bad += same_bits(sqrt32_rn_normal(x), want) ? 0 : 1;
    if (PASS == 1) raw += same_bits(__builtin_amdgcn_sqrtf(x), want) ? 0 : 1;
  }
  if (n) atomicAdd(&c[0], n);
  if (bad) atomicAdd(&c[1], bad);
  if (out) atomicAdd(&c[2], out);
  if (raw) atomicAdd(&c[3], raw);
}

int main() {
  unsigned long long* d;
  unsigned long long h1[4], h2[4];
  if (hipMalloc(&d, 64) != hipSuccess) return 5;
  if (hipMemset(d, 0, 64) != hipSuccess) return 5;
  hipLaunchKernelGGL(k_check<1>, dim3(4096), dim3(256), 0, 0, (unsigned long long)kLo, (unsigned long long)(kHi - kLo) + 1ull, d);
  hipLaunchKernelGGL(k_check<2>, dim3(4096), dim3(256), 0, 0, 0ull, 1ull << 32, d + 4);
  if (hipGetLastError() != hipSuccess) return 6;
  if (hipMemcpy(h1, d, 32, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h2, d + 4, 32, hipMemcpyDeviceToHost) != hipSuccess) return 7;
  printf("sqrt32 range %llu %llu\n", h1[0], h1[1]);
  printf("sqrt32 radius %llu %llu %llu\n", h2[0], h2[1], h2[2]);
  printf("sqrt32 estimate %llu\n", h1[3]);
  printf("sqrt32_check done\n");
  (void)hipFree(d);
  return 0;
}
