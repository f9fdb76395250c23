// mtg_host_evaluate_at.cpp -- host (CPU) path of mtg_evaluate_at_batch: mtg_host_evaluate_at_batch,
// the reference's Trajectory::evaluate (src/trajectory.cpp:41-66) over Polynomial::evaluate
// (polynomial.h:120-151) at caller-given times, followed literally: the linear scan of the
// accumulated segment times, t - (acc - T_i), multiply-then-add Horner steps.  Product code for single
// trajectories and the bitwise comparator of the kernels (mtg_evaluate_at.hip).  This file must not be
// compiled with FMA contraction (the project builds its host code with -ffp-contract=off; the pragma
// below says so again for any other build).
#include <cfloat>
#include <cmath>
#include <limits>
#include <vector>

#include "mtg.h"
#include "mtg_host_threads.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace {

// Polynomial::base_coefficients_(k, j) = j!/(j-k)! (src/polynomial.cpp:140-155), exact in a double
double base_coeff(int k, int j) {
  if (j < k) return 0.0;
  double out = 1.0;
  for (int i = j - k + 1; i <= j; ++i) out *= (double)i;
  return out;
}

// one trajectory: coeffs [K][D][N], times [K], tq [M] -> out [M][nd][D], in_range [M]
int one(int N, int D, int K, const double* coeffs, const double* times, const double* tq, int64_t M, int k0, int nd,
        const double (*base)[12], double* out, uint8_t* in_range) {
  const int W = nd * D;
  bool bad = false;
  for (int i = 0; i < K; ++i) bad = bad || !(times[i] > 0.0 && times[i] <= DBL_MAX);
  for (int64_t m = 0; m < M; ++m) {
    const double t = tq[m];
    double* row = out + m * W;
    double acc = 0.0;
    int i = 0;
    for (i = 0; i < K; ++i) {
      acc = acc + times[i];
      if (acc > t) break;
    }
    const bool beyond = t > acc;
    const bool nan = bad || t != t;
    if (in_range) in_range[m] = !(nan || beyond);
    if (nan || beyond) {
      for (int j = 0; j < W; ++j) row[j] = nan ? std::numeric_limits<double>::quiet_NaN() : 0.0;
      continue;
    }
    if (i == K) i = K - 1;  // t equal to the total: the last segment (the reference indexes past it)
    const double before = acc - times[i];
    const double tl = t - before;
    for (int q = 0; q < nd; ++q) {
      const int k = k0 + q;
      for (int d = 0; d < D; ++d) {
        double r = 0.0;
        if (k < N) {
          const double* c = coeffs + ((size_t)i * D + d) * N;
          r = base[k][N - 1] * c[N - 1];
          for (int j = N - 2; j >= k; --j) {
            r = r * tl;
            const double term = base[k][j] * c[j];
            r = r + term;
          }
        }
        row[q * D + d] = r;
      }
    }
  }
  return bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
}

}  // namespace

extern "C" int mtg_host_evaluate_at_batch(int N, int D, int K, int64_t batch, const double* coeffs, const double* times,
                                          const double* t_query, int64_t t_stride, int64_t M, int derivative_begin,
                                          int n_derivatives, double* out, uint8_t* in_range_out, int32_t* status,
                                          int threads) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (K < 1 || D < 1 || batch < 0 || M < 0) return MTG_ERR_SIZE_MISMATCH;
  if (derivative_begin < 0 || n_derivatives < 1 || n_derivatives > N) return MTG_ERR_BAD_DERIVATIVE;
  if (t_stride < 0 || (t_stride > 0 && t_stride < M)) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0 || M == 0) return MTG_OK;
  if (!coeffs || !times || !t_query || !out) return MTG_ERR_INVALID_ARGUMENT;
  double base[12][12];
  for (int k = 0; k < 12; ++k)
    for (int j = 0; j < 12; ++j) base[k][j] = base_coeff(k, j);
  const size_t sc = (size_t)K * D * N, so = (size_t)M * n_derivatives * D;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) {
      const int st = one(N, D, K, coeffs + b * sc, times + b * K, t_query + b * t_stride, M, derivative_begin,
                         n_derivatives, base, out + b * so, in_range_out ? in_range_out + b * M : nullptr);
      if (status) status[b] = st;
    }
  });
  return MTG_OK;
}

// Host path of mtg_evaluate_at_ragged_batch: the same scalar code on each trajectory's blocks of the
// CSR arrays, threaded over trajectories.
extern "C" int mtg_host_evaluate_at_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                                 const double* coeffs, const double* times, const double* t_query,
                                                 int64_t t_stride, int64_t M, int derivative_begin, int n_derivatives,
                                                 double* out, uint8_t* in_range_out, int32_t* status, int threads) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D < 1 || batch < 0 || M < 0) return MTG_ERR_SIZE_MISMATCH;
  if (derivative_begin < 0 || n_derivatives < 1 || n_derivatives > N) return MTG_ERR_BAD_DERIVATIVE;
  if (t_stride < 0 || (t_stride > 0 && t_stride < M)) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!seg_count) return MTG_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> so((size_t)batch + 1, 0);
  for (int64_t b = 0; b < batch; ++b) {
    if (seg_count[b] < 1) return MTG_ERR_SIZE_MISMATCH;
    so[(size_t)b + 1] = so[(size_t)b] + seg_count[b];
  }
  if (M == 0) return MTG_OK;
  if (!coeffs || !times || !t_query || !out) return MTG_ERR_INVALID_ARGUMENT;
  double base[12][12];
  for (int k = 0; k < 12; ++k)
    for (int j = 0; j < 12; ++j) base[k][j] = base_coeff(k, j);
  const size_t DN = (size_t)D * N, row = (size_t)M * n_derivatives * D;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) {
      const size_t s0 = (size_t)so[(size_t)b];
      const int st = one(N, D, seg_count[b], coeffs + s0 * DN, times + s0, t_query + b * t_stride, M, derivative_begin,
                         n_derivatives, base, out + b * row, in_range_out ? in_range_out + b * M : nullptr);
      if (status) status[b] = st;
    }
  });
  return MTG_OK;
}
