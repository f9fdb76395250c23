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
#include <limits>
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

// ---- Host paths of mtg_segment_min_max_magnitude_batch / mtg_segment_min_max_axis_batch: one search
// per segment (magnitude) or per (segment, dimension) (axis) on its window, the candidate list kept.
namespace {

constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();

struct SegmentArgs {
  int N, D, k, cap;
  const double *coeffs, *times, *windows;
  mtg_extremum *mn, *mx;
  double* cand;
  int32_t *count, *status;
};

// the window of segment s; false: MTG_TRAJ_BAD_TIME
bool segment_window(const SegmentArgs& a, int64_t s, double* t0, double* t1) {
  if (a.windows) {
    *t0 = a.windows[2 * s], *t1 = a.windows[2 * s + 1];
    return std::isfinite(*t0) && std::isfinite(*t1) && *t0 <= *t1;
  }
  *t0 = 0.0, *t1 = a.times[s];
  return *t1 > 0.0 && std::isfinite(*t1);
}

// one item: segment s, output slot `item`; axis >= 0: the signed value of that dimension
void segment_item(const SegmentArgs& a, int64_t s, int64_t item, unsigned dims, int axis, double* f, double* q,
                  double* q1, std::vector<double>* roots) {
  double t0, t1;
  const bool ok = segment_window(a, s, &t0, &t1);
  double* row = a.cand ? a.cand + item * a.cap : nullptr;
  if (!ok) {  // every floating output NaN, the count 0
    if (a.mn) a.mn[item] = mtg_extremum{kNaN, kNaN, 0, 0};
    if (a.mx) a.mx[item] = mtg_extremum{kNaN, kNaN, 0, 0};
    for (int e = 0; row && e < a.cap; ++e) row[e] = kNaN;
    if (a.count) a.count[item] = 0;
    return;
  }
  const double* cs = a.coeffs + (size_t)s * a.D * a.N;
  roots->clear();
  mtg::HostExt lo, hi;
  auto sink = [&](double t) { roots->push_back(t); };
  int lf;
  if (axis >= 0)
    lf = mtg::host_segment_extrema_on<true>(
        a.N, a.D, cs, t0, t1, a.k, dims, mtg::SegmentCandidates::kBothEnds, f, q, q1,
        [&](double t) { return mtg::host_segment_axis_value(a.N, cs, axis, a.k, t); }, sink, &lo, &hi);
  else
    lf = mtg::host_segment_extrema_on<true>(
        a.N, a.D, cs, t0, t1, a.k, dims, mtg::SegmentCandidates::kBothEnds, f, q, q1,
        [&](double t) { return mtg::host_segment_magnitude(a.N, a.D, cs, a.k, dims, t); }, sink, &lo, &hi);
  bool zero_f = true;  // the zero polynomial has no roots (rpoly.cpp:62-65): the list is the two ends
  for (int j = 0; j < lf; ++j) zero_f = zero_f && f[j] == 0.0;
  if (zero_f) roots->clear();
  if (a.mn) a.mn[item] = mtg_extremum{lo.t, lo.v, 0, 0};
  if (a.mx) a.mx[item] = mtg_extremum{hi.t, hi.v, 0, 0};
  if (a.count) a.count[item] = (int32_t)(2 + roots->size());
  if (row) {
    row[0] = t0, row[1] = t1;
    for (int e = 2; e < a.cap; ++e) row[e] = (size_t)(e - 2) < roots->size() ? (*roots)[e - 2] : 0.0;
  }
}

int segment_check(int N, int D, int64_t S, const double* coeffs, const double* times, const double* windows,
                  int derivative, uint32_t dimension_mask, const double* cand, int cap, uint32_t* dims) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D < 1 || S < 0) return MTG_ERR_SIZE_MISMATCH;
  if (derivative < 0 || derivative > N - 2) return MTG_ERR_BAD_DERIVATIVE;
  const uint32_t all = D >= 32 ? 0xffffffffu : ((1u << D) - 1u);
  *dims = dimension_mask ? dimension_mask : all;
  if (D > 32 || (*dims & ~all)) return MTG_ERR_INVALID_ARGUMENT;
  if (cand && cap < 2) return MTG_ERR_INVALID_ARGUMENT;
  if (S > 0 && (!coeffs || (!times && !windows))) return MTG_ERR_INVALID_ARGUMENT;
  return MTG_OK;
}

}  // namespace

extern "C" int mtg_host_segment_min_max_magnitude_batch(int N, int D, int64_t n_segments, const double* coeffs,
                                                        const double* times, const double* windows, int derivative,
                                                        uint32_t dimension_mask, mtg_extremum* minimum,
                                                        mtg_extremum* maximum, double* candidate_times,
                                                        int32_t* candidate_count, int candidate_capacity,
                                                        int32_t* status, int threads) {
  uint32_t dims;
  if (int rc = segment_check(N, D, n_segments, coeffs, times, windows, derivative, dimension_mask, candidate_times,
                             candidate_capacity, &dims))
    return rc;
  const SegmentArgs a{N,       D,       derivative,      candidate_capacity, coeffs, times, windows,
                      minimum, maximum, candidate_times, candidate_count,    status};
  mtg::run_threads(n_segments, threads, [&](int64_t s0, int64_t s1) {
    std::vector<double> f(2 * N), q(N), q1(N), roots;
    for (int64_t s = s0; s < s1; ++s) {
      double t0, t1;
      if (status) status[s] = segment_window(a, s, &t0, &t1) ? MTG_TRAJ_OK : MTG_TRAJ_BAD_TIME;
      segment_item(a, s, s, dims, -1, f.data(), q.data(), q1.data(), &roots);
    }
  });
  return MTG_OK;
}

extern "C" int mtg_host_segment_min_max_axis_batch(int N, int D, int64_t n_segments, const double* coeffs,
                                                   const double* times, const double* windows, int derivative,
                                                   mtg_extremum* minimum, mtg_extremum* maximum,
                                                   double* candidate_times, int32_t* candidate_count,
                                                   int candidate_capacity, int32_t* status, int threads) {
  uint32_t dims;
  if (int rc = segment_check(N, D, n_segments, coeffs, times, windows, derivative, 0, candidate_times,
                             candidate_capacity, &dims))
    return rc;
  const SegmentArgs a{N,       D,       derivative,      candidate_capacity, coeffs, times, windows,
                      minimum, maximum, candidate_times, candidate_count,    status};
  mtg::run_threads(n_segments, threads, [&](int64_t s0, int64_t s1) {
    std::vector<double> f(2 * N), q(N), q1(N), roots;
    for (int64_t s = s0; s < s1; ++s) {
      double t0, t1;
      if (status) status[s] = segment_window(a, s, &t0, &t1) ? MTG_TRAJ_OK : MTG_TRAJ_BAD_TIME;
      for (int d = 0; d < D; ++d) segment_item(a, s, s * D + d, 1u << d, d, f.data(), q.data(), q1.data(), &roots);
    }
  });
  return MTG_OK;
}
