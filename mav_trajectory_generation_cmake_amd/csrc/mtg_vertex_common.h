// mtg_vertex_common.h -- the per-item arithmetic of the two vertex <-> coefficient maps, shared by the
// uniform kernels (mtg_vertex.hip), the CSR kernels (mtg_vertex_ragged.hip) and mtg_soft_constraint.hip,
// so that an item's bits do not depend on the kernel that computes it.
//
// coefficients_from_ends: coefficients of one (segment, dimension) from the derivatives at its two ends,
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

// falling factorial k!/(k-n)! (Polynomial::base_coefficients_, src/polynomial.cpp:140-155)
__device__ __forceinline__ double falling(int k, int n) {
  double f = 1.0;
  for (int q = 0; q < n; ++q) f *= (double)(k - q);
  return f;
}

// vertex_derivative_from_ends: derivative k of one dimension at one vertex, the reference's M^+ A p
// (nl_impl:162-180): the mean of the two segment ends that meet at an interior vertex, the single end at
// the first / last vertex of a trajectory.  cstart(j): coefficient j of the segment that starts at the
// vertex (called when at_start); cend(j) and tend(): coefficient j and the time of the segment that ends
// there (called when at_end).  At least one of the two holds.
template <int N, class CStart, class CEnd, class TEnd>
__device__ __forceinline__ double vertex_derivative_from_ends(bool at_start, bool at_end, int k, CStart cstart,
                                                              CEnd cend, TEnd tend) {
  double sum = 0.0;
  int cnt = 0;
  if (at_start) {  // start of the segment: p^(k)(0) = k! c_k
    sum += falling(k, k) * cstart(k);
    ++cnt;
  }
  if (at_end) {  // end of the segment before: p^(k)(T) = sum_j j!/(j-k)! c_j T^(j-k)  (Horner)
    const double T = tend();
    double acc = 0.0;
    for (int j = N - 1; j >= k; --j) acc = acc * T + falling(j, k) * cend(j);
    sum += acc;
    ++cnt;
  }
  return cnt == 2 ? 0.5 * sum : sum;
}

// dst[i] = src[i] for i < n by a block of kVtxThreads, U loads per thread in flight before the stores.
constexpr int kVtxThreads = 256;
template <int U>
__device__ __forceinline__ void stage_copy(const double* __restrict__ src, double* dst, int n, int tid) {
  for (int base = 0; base < n; base += U * kVtxThreads) {
    double r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * kVtxThreads + tid;
      r[u] = src[i < n ? i : n - 1];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * kVtxThreads + tid;
      if (i < n) dst[i] = r[u];
    }
  }
}

}  // namespace mtg
