// layout_check.cpp -- host-only check of the layout transposition behind the C API's host-pointer entry points (no HIP, no GPU):
// to_soa / from_soa round-trip every block exactly, put every element where the layout says, and copy SoA input verbatim.
//   g++ -std=c++17 -fsanitize=address,undefined tests/c/layout_check.cpp -o layout_check && ./layout_check
#include "../../rome.jl_amd/csrc/rome_layout.h"

#include <cstdio>
#include <vector>

static int check(int C, int N, int d) {
  const size_t cnt = (size_t)C * N * d;
  std::vector<double> src(cnt + 1), soa(cnt + 1, -1.0), back(cnt + 1, -2.0);   // (+ 1: a sentinel behind the data, non-null for C = 0)
  for (size_t i = 0; i <= cnt; ++i) src[i] = 1.0 + (double)i * 0.37;           // all different
  const double s_soa = soa[cnt], s_back = back[cnt];
  int bad = 0;
  for (int layout : {ROME_LAYOUT_SOA, ROME_LAYOUT_AOS}) {
    rome::to_soa(src.data(), C, N, d, layout, soa.data());
    for (int c = 0; c < C; ++c)
      for (int i = 0; i < N; ++i)
        for (int k = 0; k < d; ++k) {
          const size_t at_soa = ((size_t)c * d + k) * N + i, at_aos = ((size_t)c * N + i) * d + k;
          bad += soa[at_soa] != src[layout == ROME_LAYOUT_SOA ? at_soa : at_aos];   // SoA in: a plain copy
        }
    rome::from_soa(soa.data(), C, N, d, layout, back.data());
    for (size_t i = 0; i < cnt; ++i) bad += back[i] != src[i];
    bad += soa[cnt] != s_soa || back[cnt] != s_back;   // nothing written past the blocks
  }
  if (bad) std::printf("layout_check: C=%d N=%d d=%d: %d mismatches\n", C, N, d, bad);
  return bad;
}

int main() {
  int bad = 0;
  for (int C : {0, 1, 3}) for (int N : {1, 2, 33}) for (int d : {1, 2, 3, 6}) bad += check(C, N, d);
  bad += rome::point_len(2) != 2 || rome::point_len(3) != 6 || rome::point_len(6) != 12;
  if (!bad) std::printf("layout_check ok\n");
  return bad ? 1 : 0;
}
