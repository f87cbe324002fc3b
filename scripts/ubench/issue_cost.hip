// issue cost of the instruction classes of the packed sweep's stream on gfx950, 8 waves per SIMD resident: SIMD-cycles per wave-instruction.
// Each class is one instruction in inline assembly on eight independent register chains per lane (nothing for the compiler to fold);
// the loop overhead (one s_add, one s_cmp, one branch per 8 instructions) is scalar.  (v_cndmask_b32 reads a vcc that no VALU instruction
// wrote: it read 18.9 cycles in this form, which is not understood -- profiles/trim_issue_cost.txt -- and is not used anywhere.)
//   hipcc --offload-arch=gfx950 -O3 -o scripts/ubench/issue_cost scripts/ubench/issue_cost.hip && scripts/ubench/issue_cost
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define ITERS 512
enum { FMA32, PKFMA32, SQRT32, CVT64, FMA64, MUL64, MAD64, LSHLADD64, MULLO, CNDMASK, BITOP3, MOV, NCLASS };
static const char* kNames[NCLASS] = {"v_fma_f32", "v_pk_fma_f32", "v_sqrt_f32", "v_cvt_f64_f32", "v_fma_f64", "v_mul_f64", "v_mad_u64_u32", "v_lshl_add_u64",
                                     "v_mul_lo_u32", "v_cndmask_b32", "v_bitop3_b32", "v_mov_b32"};

template <int WHICH>
__global__ void __launch_bounds__(256) k(float* out, float seed) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  float a[8];
  double d[8];
  uint64_t q[8];
  uint32_t w[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    a[u] = seed * (float)(tid & 63) * 1e-3f + (float)(u + 1);
    d[u] = (double)a[u]; q[u] = (uint64_t)(tid + u) * 0x9E3779B97F4A7C15ull; w[u] = (uint32_t)(tid * 2654435761u + u);
  }
  const float b = seed * 0.999f, c = seed * 0.25f;
  const double bd = (double)b, cd = (double)c;
  const uint32_t wb = (uint32_t)tid | 1u;
  for (int i = 0; i < ITERS; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if constexpr (WHICH == FMA32) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[u]) : "v"(b), "v"(c));
      if constexpr (WHICH == PKFMA32) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(d[u]) : "v"(bd), "v"(cd));   // (a register pair as two floats)
      if constexpr (WHICH == SQRT32) asm volatile("v_sqrt_f32 %0, %0" : "+v"(a[u]));
      if constexpr (WHICH == CVT64) asm volatile("v_cvt_f64_f32 %0, %1" : "+v"(d[u]) : "v"(a[u]));
      if constexpr (WHICH == FMA64) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[u]) : "v"(bd), "v"(cd));
      if constexpr (WHICH == MUL64) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(d[u]) : "v"(bd));
      if constexpr (WHICH == MAD64) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(q[u]) : "v"(w[u]), "v"(wb) : "vcc");
      if constexpr (WHICH == LSHLADD64) asm volatile("v_lshl_add_u64 %0, %0, 1, %1" : "+v"(q[u]) : "v"(q[(u + 1) & 7]));
      if constexpr (WHICH == MULLO) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(w[u]) : "v"(wb));
      if constexpr (WHICH == CNDMASK) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(w[u]) : "v"(wb) : "vcc");
      if constexpr (WHICH == BITOP3) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(w[u]) : "v"(wb), "v"(w[(u + 1) & 7]));
      if constexpr (WHICH == MOV) asm volatile("v_mov_b32 %0, %1" : "+v"(w[u]) : "v"(wb));
    }
  }
  float acc = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) acc += a[u] + (float)d[u] + (float)(q[u] >> 40) + (float)w[u];
  out[tid] = acc;
}
template <int W> static float run(float* d, int blocks) {
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0f;
  hipLaunchKernelGGL((k<W>), dim3(blocks), dim3(256), 0, 0, d, 1.0f);
  if (hipDeviceSynchronize() != hipSuccess) return -1.0f;
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {
    (void)hipEventRecord(e0); hipLaunchKernelGGL((k<W>), dim3(blocks), dim3(256), 0, 0, d, 1.0f); (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) return -1.0f;
    float ms; (void)hipEventElapsedTime(&ms, e0, e1); best = ms < best ? ms : best;
  }
  return best;
}
int main() {
  const int blocks = 256 * 8 * 4;   // 8 waves per SIMD, four generations
  float* d;
  if (hipMalloc(&d, sizeof(float) * (size_t)blocks * 256) != hipSuccess) return 5;
  const float ms[NCLASS] = {run<FMA32>(d, blocks), run<PKFMA32>(d, blocks), run<SQRT32>(d, blocks), run<CVT64>(d, blocks), run<FMA64>(d, blocks), run<MUL64>(d, blocks),
                            run<MAD64>(d, blocks), run<LSHLADD64>(d, blocks), run<MULLO>(d, blocks), run<CNDMASK>(d, blocks), run<BITOP3>(d, blocks), run<MOV>(d, blocks)};
  const double waves_per_simd = blocks * 4.0 / 1024.0;
  for (int i = 0; i < NCLASS; ++i)
    printf("%-16s %8.3f ms -> %6.2f SIMD-cycles per wave-instruction (2.4 GHz)\n", kNames[i], ms[i], ms[i] * 2.4e6 / (ITERS * 8.0 * waves_per_simd));
  (void)hipFree(d);
  return 0;
}
