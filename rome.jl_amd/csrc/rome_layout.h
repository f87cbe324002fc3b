// rome_layout.h -- host transposition between the caller's block layouts and SoA (a copy: no arithmetic).  No HIP: a host-only
// program compiles it (tests/c/layout_check.cpp).
#pragma once
#include "../../include/rome_mi355.h"

#include <cstddef>
#include <cstring>

namespace rome {

inline int point_len(int dim) { return dim == 3 ? 6 : (dim == 6 ? 12 : dim); }

// host blocks [C][N][d] (AoS) or [C][d][N] (SoA)  ->  SoA
inline void to_soa(const double* src, int C, int N, int d, int layout, double* dst) {
  if (layout == ROME_LAYOUT_SOA) { std::memcpy(dst, src, (size_t)C * N * d * sizeof(double)); return; }
  for (int c = 0; c < C; ++c) {
    const double* s = src + (size_t)c * N * d; double* o = dst + (size_t)c * N * d;
    for (int i = 0; i < N; ++i) for (int k = 0; k < d; ++k) o[(size_t)k * N + i] = s[(size_t)i * d + k];
  }
}
inline void from_soa(const double* src, int C, int N, int d, int layout, double* dst) {
  if (layout == ROME_LAYOUT_SOA) { std::memcpy(dst, src, (size_t)C * N * d * sizeof(double)); return; }
  for (int c = 0; c < C; ++c) {
    const double* s = src + (size_t)c * N * d; double* o = dst + (size_t)c * N * d;
    for (int i = 0; i < N; ++i) for (int k = 0; k < d; ++k) o[(size_t)i * d + k] = s[(size_t)k * N + i];
  }
}

}  // namespace rome
