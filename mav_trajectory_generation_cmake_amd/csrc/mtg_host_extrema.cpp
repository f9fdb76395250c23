// mtg_host_extrema.cpp -- host (CPU) path of mtg_min_max_magnitude_batch:
// mtg_host_min_max_magnitude_batch, the reference's Trajectory::computeMinMaxMagnitude
// (src/trajectory.cpp:181-218) for the drop-in's single trajectories, which the reference also
// computes on the CPU.  Same algorithm as the HIP kernel (mtg_extrema.hip; the segment search is
// mtg_host_extrema_common.h, shared with mtg_host_soft_constraint.cpp): per segment the
// candidates t = 0, t = T and the real roots in [0, T] of sum_d conv(p_d^(k), p_d^(k+1)) (one
// dimension: of p^(k+1)), isolated by sign changes on 256 uniform samples and refined by safeguarded
// Newton-bisection; the magnitude at each candidate; the first candidate / segment wins ties.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <thread>
#include <vector>

#include "mtg.h"
#include "mtg_host_extrema_common.h"
#include "mtg_host_threads.h"

namespace {

// one trajectory: coeffs [K][D][N], times [K]
void one(int N, int D, int K, const double* coeffs, const double* times, int k, unsigned dims, mtg_extremum* out_min,
         mtg_extremum* out_max) {
  mtg::HostExt m{0.0, DBL_MAX}, M{0.0, -DBL_MAX};
  int im = 0, iM = 0;
  std::vector<double> f(2 * N), q(N), q1(N);
  for (int i = 0; i < K; ++i) {
    mtg::HostExt lo, hi;
    mtg::host_segment_extrema(N, D, coeffs + (size_t)i * D * N, times[i], k, dims, mtg::SegmentCandidates::kBothEnds,
                              f.data(), q.data(), q1.data(), &lo, &hi);
    if (i == 0 || lo.v < m.v) m = lo, im = i;  // strict: the first segment wins ties
    if (i == 0 || hi.v > M.v) M = hi, iM = i;
  }
  if (out_min) *out_min = mtg_extremum{m.t, m.v, im, 0};
  if (out_max) *out_max = mtg_extremum{M.t, M.v, iM, 0};
}

}  // namespace

extern "C" int mtg_host_min_max_magnitude_batch(int N, int D, int K, int64_t batch, const double* coeffs,
                                                const double* times, int derivative, uint32_t dimension_mask,
                                                mtg_extremum* minimum, mtg_extremum* maximum, int threads) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (K < 1 || D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (derivative < 0 || derivative > N - 2) return MTG_ERR_BAD_DERIVATIVE;
  const uint32_t all = D >= 32 ? 0xffffffffu : ((1u << D) - 1u);
  const uint32_t dims = dimension_mask ? dimension_mask : all;
  if (D > 32 || (dims & ~all)) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!coeffs || !times) return MTG_ERR_INVALID_ARGUMENT;
  const size_t sc = (size_t)K * D * N;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b)
      one(N, D, K, coeffs + b * sc, times + b * K, derivative, dims, minimum ? minimum + b : nullptr,
          maximum ? maximum + b : nullptr);
  });
  return MTG_OK;
}

// Host path of mtg_min_max_magnitude_ragged_batch: the same scalar code on each trajectory's blocks of
// the CSR arrays, threaded over trajectories.
extern "C" int mtg_host_min_max_magnitude_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                                       const double* coeffs, const double* times, int derivative,
                                                       uint32_t dimension_mask, mtg_extremum* minimum,
                                                       mtg_extremum* maximum, int threads) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (derivative < 0 || derivative > N - 2) return MTG_ERR_BAD_DERIVATIVE;
  const uint32_t all = D >= 32 ? 0xffffffffu : ((1u << D) - 1u);
  const uint32_t dims = dimension_mask ? dimension_mask : all;
  if (D > 32 || (dims & ~all)) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!seg_count) return MTG_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> so((size_t)batch + 1, 0);
  for (int64_t b = 0; b < batch; ++b) {
    if (seg_count[b] < 1) return MTG_ERR_SIZE_MISMATCH;
    so[(size_t)b + 1] = so[(size_t)b] + seg_count[b];
  }
  if (!coeffs || !times) return MTG_ERR_INVALID_ARGUMENT;
  const size_t DN = (size_t)D * N;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) {
      const size_t s0 = (size_t)so[(size_t)b];
      one(N, D, seg_count[b], coeffs + s0 * DN, times + s0, derivative, dims, minimum ? minimum + b : nullptr,
          maximum ? maximum + b : nullptr);
    }
  });
  return MTG_OK;
}
