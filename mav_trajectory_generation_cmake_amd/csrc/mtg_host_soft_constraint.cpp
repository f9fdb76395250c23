// mtg_host_soft_constraint.cpp -- host (CPU) path of mtg_soft_constraint_cost_batch: the reference's
// getCostAndGradientSoftConstraints (polynomial_optimization_nonlinear_impl.h:2025-2091) over
// evaluateMaximumMagnitudeAsSoftConstraint (:2396-2425) and
// PolynomialOptimization::computeMaximumOfMagnitude (lin_impl:470-503), written literally: for every
// (dimension, free derivative, side) the vertex values are perturbed, ALL coefficients re-formed
// (setFreeConstraints) and ALL segments searched.  No use of the fact that a perturbation touches two
// segments: this path is what the kernel's shortcut is checked against.  The segment search is
// mtg_host_extrema_common.h, shared with mtg_host_extrema.cpp.  Plain C++ (no HIP).
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

struct Work {
  std::vector<double> x, coeffs, f, q, q1;
};

// computeMaximumOfMagnitude<k>: per segment t = 0 and the roots, after the last segment t = T_K; a
// candidate replaces the best only when strictly larger
mtg_extremum maximum_of_magnitude(int N, int D, int K, const double* coeffs, const double* times, int k, Work& w) {
  const unsigned dims = (1u << D) - 1u;
  mtg_extremum best{0.0, 0.0, 0, 0};  // Extremum(): time 0, value 0, segment 0 (extremum.h)
  for (int i = 0; i < K; ++i) {
    mtg::HostExt lo, hi;
    mtg::host_segment_extrema(N, D, coeffs + (size_t)i * D * N, times[i], k, dims, mtg::SegmentCandidates::kStartOnly,
                              w.f.data(), w.q.data(), w.q1.data(), &lo, &hi);
    if (hi.v > best.value) best = mtg_extremum{hi.t, hi.v, i, 0};
  }
  const double vT = mtg::host_segment_magnitude(N, D, coeffs + (size_t)(K - 1) * D * N, k, dims, times[K - 1]);
  if (vT > best.value) best = mtg_extremum{times[K - 1], vT, K - 1, 0};
  return best;
}

// evaluateMaximumMagnitudeAsSoftConstraint at vertex values x
double soft_cost(int N, int D, int K, const double* x, const double* times, const mtg_soft_constraint_params& p,
                 mtg_extremum* maxima, Work& w) {
  mtg_host_coefficients_from_vertices_batch(N, D, K, 1, x, times, w.coeffs.data(), 1);
  double cost = 0.0;
  for (int c = 0; c < p.n_constraints; ++c) {
    const mtg_extremum m = maximum_of_magnitude(N, D, K, w.coeffs.data(), times, p.derivative[c], w);
    if (maxima) maxima[c] = m;
    const double abs_violation = m.value - p.limit[c];
    const double relative_violation = abs_violation / p.limit[c];
    const double e = std::exp(relative_violation * p.weight);
    cost += e < p.maximum_cost ? e : p.maximum_cost;  // std::min(maximum_cost, e)
  }
  return cost;
}

void one(int N, int D, int K, const double* values, const uint8_t* mask, const double* times,
         const mtg_soft_constraint_params& p, double* cost, double* grad, mtg_extremum* maxima, int32_t* status,
         Work& w) {
  const int h = N / 2, V = K + 1;
  bool bad = false;
  for (int i = 0; i < K; ++i)
    if (!(times[i] > 0.0 && times[i] <= DBL_MAX)) bad = true;
  if (grad) std::fill(grad, grad + (size_t)D * V * h, 0.0);
  if (status) *status = bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
  if (bad) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    *cost = nan;
    if (maxima)
      for (int c = 0; c < p.n_constraints; ++c) maxima[c] = mtg_extremum{nan, nan, 0, 0};
    return;
  }
  w.coeffs.resize((size_t)K * D * N);
  w.f.resize(2 * N);
  w.q.resize(N);
  w.q1.resize(N);
  if (grad) {
    w.x.assign(values, values + (size_t)V * h * D);
    const unsigned hm = (1u << h) - 1u;
    const double inc = p.increment;
    for (int d = 0; d < D; ++d) {
      double* g = grad + (size_t)d * V * h;
      int n = 0;
      for (int v = 0; v <= K; ++v)
        for (int k = 0; k < h; ++k) {
          if (((mask[v] & hm) >> k) & 1u) continue;
          double& xv = w.x[((size_t)v * h + k) * D + d];
          const double x0 = xv;
          xv = x0 - inc;
          const double cost_left = soft_cost(N, D, K, w.x.data(), times, p, nullptr, w);
          xv = x0 + inc;
          const double cost_right = soft_cost(N, D, K, w.x.data(), times, p, nullptr, w);
          xv = x0;
          g[n++] = (cost_right - cost_left) / (2.0 * inc);
        }
    }
  }
  *cost = soft_cost(N, D, K, values, times, p, maxima, w);
}

}  // namespace

extern "C" int mtg_host_soft_constraint_cost_batch(int N, int D, int K, int64_t batch, const double* vertex_values,
                                                   const uint8_t* fixed_mask, const double* times,
                                                   const mtg_soft_constraint_params* params, double* cost_out,
                                                   double* grad_out, mtg_extremum* maxima_out, int32_t* status,
                                                   int threads) {
  if (N < 6 || N > 12 || (N % 2)) return MTG_ERR_INVALID_ARGUMENT;
  if (D < 1 || D > 4) return MTG_ERR_INVALID_ARGUMENT;
  if (K < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (!params || params->n_constraints < 1 || params->n_constraints > 8) return MTG_ERR_INVALID_ARGUMENT;
  const int kmax = N - 2 < 4 ? N - 2 : 4;
  for (int c = 0; c < params->n_constraints; ++c)
    if (params->derivative[c] < 0 || params->derivative[c] > kmax || !(params->limit[c] > 0.0))
      return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !cost_out || (grad_out && !fixed_mask)) return MTG_ERR_INVALID_ARGUMENT;
  const int h = N / 2, V = K + 1, C = params->n_constraints;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    Work w;
    for (int64_t b = b0; b < b1; ++b)
      one(N, D, K, vertex_values + b * (int64_t)V * h * D, fixed_mask ? fixed_mask + b * V : nullptr, times + b * K,
          *params, cost_out + b, grad_out ? grad_out + b * (int64_t)D * V * h : nullptr,
          maxima_out ? maxima_out + b * C : nullptr, status ? status + b : nullptr, w);
  });
  return MTG_OK;
}
