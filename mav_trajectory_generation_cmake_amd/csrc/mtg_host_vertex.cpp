// mtg_host_vertex.cpp -- host (CPU) paths of the vertex <-> coefficient maps that mtg_host_solve.cpp does
// not hold: mtg_host_vertex_derivatives_batch, the reference's M^+ A p (nl_impl:162-180) as scalar C++
// per trajectory -- the end derivatives A_i c_i of every segment (Polynomial::evaluate's Horner with the
// base coefficients j!/(j-k)!, polynomial.h:120-151), the mean of the two ends that meet at an interior
// vertex, the single end at the first / last vertex --, and the CSR forms of both maps
// (mtg_host_vertex_derivatives_ragged_batch, mtg_host_coefficients_from_vertices_ragged_batch): the
// per-trajectory code on each trajectory's blocks, threaded over trajectories.  Plain C++ (no HIP).
#include <vector>

#include "mtg.h"
#include "mtg_host_threads.h"

namespace {

// coeffs [K][D][N], times [K] -> values [K + 1][h][D]
void derivatives_one(int N, int D, int K, const double base[12][12], const double* coeffs, const double* times,
                     double* values) {
  const int h = N / 2;
  for (int v = 0; v <= K; ++v)
    for (int k = 0; k < h; ++k)
      for (int d = 0; d < D; ++d) {
        double sum = 0.0;
        int cnt = 0;
        if (v < K) {  // start of segment v: p^(k)(0) = k! c_k
          sum += base[k][k] * coeffs[((size_t)v * D + d) * N + k];
          ++cnt;
        }
        if (v > 0) {  // end of segment v - 1: p^(k)(T) by Horner
          const double T = times[v - 1];
          const double* c = coeffs + ((size_t)(v - 1) * D + d) * N;
          double acc = 0.0;
          for (int j = N - 1; j >= k; --j) acc = acc * T + base[k][j] * c[j];
          sum += acc;
          ++cnt;
        }
        values[((size_t)v * h + k) * D + d] = cnt == 2 ? 0.5 * sum : sum;
      }
}

// Polynomial::base_coefficients_(k, j) = j!/(j-k)! (src/polynomial.cpp:140-155), exact in a double
void base_table(double base[12][12]) {
  for (int k = 0; k < 12; ++k)
    for (int j = 0; j < 12; ++j) {
      double b = j < k ? 0.0 : 1.0;
      for (int i = j - k + 1; j >= k && i <= j; ++i) b *= (double)i;
      base[k][j] = b;
    }
}

// the call-level checks of the CSR forms after those on N, D and batch; so [batch + 1]
int segment_offsets(int64_t batch, const int32_t* seg_count, std::vector<int64_t>* so) {
  if (!seg_count) return MTG_ERR_INVALID_ARGUMENT;
  so->assign((size_t)batch + 1, 0);
  for (int64_t b = 0; b < batch; ++b) {
    if (seg_count[b] < 1) return MTG_ERR_SIZE_MISMATCH;
    (*so)[(size_t)b + 1] = (*so)[(size_t)b] + seg_count[b];
  }
  return MTG_OK;
}

}  // namespace

extern "C" int mtg_host_vertex_derivatives_batch(int N, int D, int K, int64_t batch, const double* coeffs,
                                                 const double* times, double* vertex_values, int threads) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (K < 1 || D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (batch == 0) return MTG_OK;
  if (!coeffs || !times || !vertex_values) return MTG_ERR_INVALID_ARGUMENT;
  double base[12][12];
  base_table(base);
  const size_t sc = (size_t)K * D * N, sv = (size_t)(K + 1) * (N / 2) * D;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) derivatives_one(N, D, K, base, coeffs + b * sc, times + b * K, vertex_values + b * sv);
  });
  return MTG_OK;
}

extern "C" int mtg_host_vertex_derivatives_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                                        const double* coeffs, const double* times,
                                                        double* vertex_values, int threads) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (batch == 0) return MTG_OK;
  std::vector<int64_t> so;
  if (int rc = segment_offsets(batch, seg_count, &so)) return rc;
  if (!coeffs || !times || !vertex_values) return MTG_ERR_INVALID_ARGUMENT;
  double base[12][12];
  base_table(base);
  const size_t DN = (size_t)D * N, hD = (size_t)(N / 2) * D;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) {
      const size_t s0 = (size_t)so[(size_t)b];
      derivatives_one(N, D, seg_count[b], base, coeffs + s0 * DN, times + s0, vertex_values + (s0 + (size_t)b) * hD);
    }
  });
  return MTG_OK;
}

extern "C" int mtg_host_coefficients_from_vertices_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                                                const double* vertex_values, const double* times,
                                                                double* coeffs, int threads) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (batch == 0) return MTG_OK;
  std::vector<int64_t> so;
  if (int rc = segment_offsets(batch, seg_count, &so)) return rc;
  if (!vertex_values || !times || !coeffs) return MTG_ERR_INVALID_ARGUMENT;
  const size_t DN = (size_t)D * N, hD = (size_t)(N / 2) * D;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) {
      const size_t s0 = (size_t)so[(size_t)b];
      mtg_host_coefficients_from_vertices_batch(N, D, seg_count[b], 1, vertex_values + (s0 + (size_t)b) * hD, times + s0,
                                                coeffs + s0 * DN, 1);
    }
  });
  return MTG_OK;
}
