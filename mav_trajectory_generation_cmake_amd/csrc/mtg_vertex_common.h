// mtg_vertex_common.h -- coefficients of one (segment, dimension) from the derivatives at its two
// ends, shared by mtg_vertex.hip (mtg_coefficients_from_vertices_batch) and mtg_soft_constraint.hip:
// c = A(T)^-1 [x_i; x_{i+1}], the reference's updateSegmentsFromCompactConstraints (lin_impl:253-273),
// with A(T)^-1 = diag(T^-j) A(1)^-1 S(T) from the exact-rational A(1)^-1 table and the segment's start
// position subtracted first (only c_0 changes; no cancellation of p_i against p_{i+1} in c_j, j >= h).
#pragma once

#include "mtg_device.h"

namespace mtg {

// xend(e, k): derivative k (< N / 2) at the segment's start (e = 0) or end (e = 1); out [N].
template <int N, class XEnd>
__device__ __forceinline__ void coefficients_from_ends(XEnd xend, double T, double* out) {
  constexpr int H = N / 2;
  const double* Ai1 = c_a1inv + MTG_A1INV_OFF(N);
  double s[H];
  s[0] = 1.0;
#pragma unroll
  for (int k = 1; k < H; ++k) s[k] = s[k - 1] * T;
  double sh[N];
#pragma unroll
  for (int k = 0; k < H; ++k) {
    sh[k] = s[k] * xend(0, k);
    sh[H + k] = s[k] * xend(1, k);
  }
  const double p0 = sh[0];
  sh[0] = 0.0;
  sh[H] -= p0;
  const double tinv = rcp(T);
  double tp = 1.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double acc;
    if (j < H) {
      acc = (j == 0) ? p0 : Ai1[j * N + j] * sh[j];
    } else {
      acc = 0.0;
#pragma unroll
      for (int q = 1; q < N; ++q) acc += Ai1[j * N + q] * sh[q];
    }
    out[j] = acc * tp;
    tp *= tinv;
  }
}

}  // namespace mtg
