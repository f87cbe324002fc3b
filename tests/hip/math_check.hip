// Unit check of the device math in rome.jl_amd/csrc/rome_device_math.hpp: evaluates every tuned elementary function on the points
// of an input file and writes the results; tests/test_gpu_device_math.py compiles this with hipcc, runs it and compares with numpy.
//   math_check <in.bin> <out.bin>     in: n doubles x, n doubles y     out: 9 arrays of n doubles
//   math_check <in.bin> <out.bin> <qin.bin> <qout.bin>   additionally the quaternion block: qin = 6 arrays of m doubles (rotation
//   vectors w1, w2), qout = kQuatOut arrays of m doubles, see k_quat
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../rome.jl_amd/csrc/rome_device_math.hpp"
using namespace rome;

__global__ void k(int n, const double* x, const double* y, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s, c; fast_sincos(x[i], &s, &c);
  o[0 * n + i] = s; o[1 * n + i] = c;
  o[2 * n + i] = wrap_pi(x[i]);
  o[3 * n + i] = fast_sqrt(fabs(x[i]));
  o[4 * n + i] = fast_log(fabs(y[i]) + 1e-300);
  o[5 * n + i] = fast_exp_neg(-fabs(x[i]));
  o[6 * n + i] = fast_atan2(y[i], x[i]);
  double w[3] = {x[i] * 0.01, y[i] * 0.01, (x[i] - y[i]) * 0.01}, q[4], back[3];
  quat_exp(w, q); quat_log(q, back);
  o[7 * n + i] = back[0] - w[0]; o[8 * n + i] = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0;
}

// The quaternion functions in full: a = quat_exp(w1), b = quat_exp(w2) ->
//   [0,4) a   [4,7) quat_log(a)   [7,11) quat_mul(a, b)   [11,15) quat_cmul(a, b)   [15,19) quat_mulc(a, b)   [19,22) quat_rot(a, w2)
//   [22,31) so3_exp(w1) (column-major)   [31,34) so3_log(so3_exp(w1))
constexpr int kQuatOut = 34;
__global__ void k_quat(int m, const double* in, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double w1[3] = {in[i], in[m + i], in[2 * m + i]}, w2[3] = {in[3 * m + i], in[4 * m + i], in[5 * m + i]};
  double a[4], b[4], l[3], p[4], v[3], R[9], r[3];
  quat_exp(w1, a); quat_exp(w2, b); quat_log(a, l);
  for (int k = 0; k < 4; ++k) o[(size_t)k * m + i] = a[k];
  for (int k = 0; k < 3; ++k) o[(size_t)(4 + k) * m + i] = l[k];
  quat_mul(a, b, p);  for (int k = 0; k < 4; ++k) o[(size_t)(7 + k) * m + i] = p[k];
  quat_cmul(a, b, p); for (int k = 0; k < 4; ++k) o[(size_t)(11 + k) * m + i] = p[k];
  quat_mulc(a, b, p); for (int k = 0; k < 4; ++k) o[(size_t)(15 + k) * m + i] = p[k];
  quat_rot(a, w2, v); for (int k = 0; k < 3; ++k) o[(size_t)(19 + k) * m + i] = v[k];
  so3_exp(w1, R);     for (int k = 0; k < 9; ++k) o[(size_t)(22 + k) * m + i] = R[k];
  so3_log(R, r);      for (int k = 0; k < 3; ++k) o[(size_t)(31 + k) * m + i] = r[k];
}
static int run_quat(const char* fin, const char* fout) {
  FILE* f = fopen(fin, "rb"); if (!f) return 3;
  fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
  const int m = (int)(bytes / 48);
  std::vector<double> h(6 * (size_t)m), out(kQuatOut * (size_t)m);
  if (fread(h.data(), 8, h.size(), f) != h.size()) return 4;
  fclose(f);
  if (m == 0) return 4;
  double *din, *dout;
  if (hipMalloc(&din, 8 * h.size()) != hipSuccess || hipMalloc(&dout, 8 * out.size()) != hipSuccess) return 5;
  if (hipMemcpy(din, h.data(), 8 * h.size(), hipMemcpyHostToDevice) != hipSuccess) return 7;
  hipLaunchKernelGGL(k_quat, dim3((m + 255) / 256), dim3(256), 0, 0, m, din, dout);
  if (hipMemcpy(out.data(), dout, 8 * out.size(), hipMemcpyDeviceToHost) != hipSuccess) return 6;
  f = fopen(fout, "wb"); if (!f) return 3;
  fwrite(out.data(), 8, out.size(), f); fclose(f);
  printf("math_check quat ok %d\n", m);
  return 0;
}

// wave64 reductions: every lane contributes 4 (and 3) values; all lanes must end with the totals
__global__ void k_wave(const double* x, double* o) {
  const int l = threadIdx.x;
  double v4[4] = {x[l], x[64 + l], x[128 + l], x[192 + l]};
  double v3[3] = {x[l], x[64 + l], x[128 + l]};
  wave_sum_n<4>(v4); wave_sum_n<3>(v3);
  for (int k = 0; k < 4; ++k) o[k * 64 + l] = v4[k];
  for (int k = 0; k < 3; ++k) o[256 + k * 64 + l] = v3[k];
}
static int check_wave(const double* dx) {
  double* dw; if (hipMalloc(&dw, 8 * 448) != hipSuccess) return 1;
  hipLaunchKernelGGL(k_wave, dim3(1), dim3(64), 0, 0, dx, dw);
  std::vector<double> w(448), in(256);
  if (hipMemcpy(w.data(), dw, 8 * 448, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (hipMemcpy(in.data(), dx, 8 * 256, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  for (int k = 0; k < 4; ++k) {
    long double ref = 0, mag = 0;
    for (int l = 0; l < 64; ++l) { ref += in[k * 64 + l]; mag += fabsl(in[k * 64 + l]); }
    for (int l = 0; l < 64; ++l) {
      if (fabsl(w[k * 64 + l] - ref) > 1e-14L * mag + 1e-300L) { printf("wave_sum_n<4> value %d lane %d: %g vs %Lg\n", k, l, w[k * 64 + l], ref); return 1; }
      if (w[k * 64 + l] != w[k * 64]) { printf("wave_sum_n<4>: lanes disagree\n"); return 1; }
      if (k < 3 && fabsl(w[256 + k * 64 + l] - ref) > 1e-14L * mag + 1e-300L) { printf("wave_sum_n<3> value %d lane %d\n", k, l); return 1; }
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
  fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
  const int n = (int)(bytes / 16);
  std::vector<double> h(2 * (size_t)n);
  if (fread(h.data(), 8, 2 * (size_t)n, f) != 2 * (size_t)n) return 4;
  fclose(f);
  double *dx, *dout;
  if (hipMalloc(&dx, 16 * (size_t)n) != hipSuccess || hipMalloc(&dout, 72 * (size_t)n) != hipSuccess) return 5;
  if (hipMemcpy(dx, h.data(), 16 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return 7;
  if (n >= 256 && check_wave(dx)) return 8;
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, n, dx, dx + n, dout);
  std::vector<double> out(9 * (size_t)n);
  if (hipMemcpy(out.data(), dout, 72 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return 6;
  f = fopen(argv[2], "wb"); fwrite(out.data(), 8, out.size(), f); fclose(f);
  printf("math_check ok %d\n", n);
  if (argc >= 5) return run_quat(argv[3], argv[4]);
  return 0;
}
