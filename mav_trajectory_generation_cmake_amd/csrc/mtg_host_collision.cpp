// mtg_host_collision.cpp -- host (CPU) path of mtg_collision_cost_batch: the reference's
// getCostAndGradientCollision (polynomial_optimization_nonlinear_impl.h:1523-1709) as one scalar
// loop in the reference's order, per trajectory.  The product with L_pp (:1677-1680) is applied
// once per segment after the loop: A(T_i)^-T on the segment's accumulated coefficient-space
// vector, then the (vertex, derivative) packing of mtg_cost_at_times_batch.  The per-position part
// (map lookup, potential, central differences) is mtg_collision_common.h, shared with the kernel.
// mtg::host_collision_cost_coeff_times is the same loop with the coefficients formed at other times
// than the loop's (the stale L_ of objectiveFunctionTime, for mtg_host_objective_time_batch).
// Plain C++ (no HIP).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <thread>
#include <vector>

#include "mtg.h"
#include "mtg_collision_common.h"
#include "mtg_host_threads.h"
#include "mtg_tables.inc"

namespace {

const double kA1inv[MTG_A1INV_SIZE] = {MTG_A1INV_VALUES};

struct Work {
  std::vector<double> coeffs;  // [K][3][N]
  std::vector<double> acc;     // [K][3][N] per-segment coefficient-space vectors
};

// coeff_times (nullable): the times the coefficients are formed at, where they differ from the loop's
void one(int N, int K, const double* values, const uint8_t* mask, const double* times, const double* coeff_times,
         const mtg::CollisionMap& map, const mtg::CollisionPot& pot, double dt, double* cost, double* grad,
         uint8_t* collision, int32_t* n_evaluated, int32_t* status, Work& w) {
  const int h = N / 2, V = K + 1, D = 3;
  bool bad = false;
  for (int i = 0; i < K; ++i) {
    const double T = times[i];
    if (!(T > 0.0 && T <= DBL_MAX) || !(T / dt <= mtg::kCollisionMaxSegmentSamples)) bad = true;
    if (coeff_times && !(coeff_times[i] > 0.0 && coeff_times[i] <= DBL_MAX)) bad = true;
  }
  if (grad) std::fill(grad, grad + (size_t)D * V * h, 0.0);
  if (collision) *collision = 0;
  if (n_evaluated) *n_evaluated = 0;
  if (status) *status = bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
  if (bad) {
    *cost = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  w.coeffs.resize((size_t)K * D * N);
  mtg_host_coefficients_from_vertices_batch(N, D, K, 1, values, coeff_times ? coeff_times : times, w.coeffs.data(), 1);
  if (grad) w.acc.assign((size_t)K * D * N, 0.0);

  double J = 0.0;
  bool is_collision = false;
  int32_t evaluated = 0;
  double prev[3] = {0.0, 0.0, 0.0};
  double time_sum = -1.0, dist_sum = 0.0;
  for (int i = 0; i < K; ++i) {
    const double T = times[i];
    double t;
    for (t = 0.0; t < T; t += dt) {
      double pos[3], vel[3];
      for (int k = 0; k < D; ++k) {
        const double* c = w.coeffs.data() + ((size_t)i * D + k) * N;
        double p = c[N - 1], v = (double)(N - 1) * c[N - 1];
        for (int n = N - 2; n >= 0; --n) p = p * t + c[n];
        for (int n = N - 2; n >= 1; --n) v = v * t + (double)n * c[n];
        pos[k] = p;
        vel[k] = v;
      }
      if (time_sum < 0) {  // numerical integration: skip the first entry
        time_sum = 0.0;
        for (int k = 0; k < D; ++k) prev[k] = pos[k];
        continue;
      }
      time_sum += dt;
      const double dx = pos[0] - prev[0], dy = pos[1] - prev[1], dz = pos[2] - prev[2];
      dist_sum += std::sqrt(dx * dx + dy * dy + dz * dz);
      for (int k = 0; k < D; ++k) prev[k] = pos[k];
      if (dist_sum < pot.increment) continue;

      double gc[3] = {0.0, 0.0, 0.0};
      bool pos_collision;
      const double c = mtg::collision_potential_at(map, pot, pos, grad != nullptr, gc, pos_collision);
      if (pos_collision) is_collision = true;
      ++evaluated;
      const double vn = std::sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]);
      J += c * vn * time_sum;
      if (grad && vn > 1e-6) {
        for (int k = 0; k < D; ++k) {
          const double a = vn * time_sum * gc[k], bq = time_sum * c * vel[k] / vn;
          double* acc = w.acc.data() + ((size_t)i * D + k) * N;
          double tp = 1.0, tm = 0.0;  // t^n, t^(n-1)
          for (int n = 0; n < N; ++n) {
            acc[n] += a * tp + bq * ((double)n * tm);
            tm = tp;
            tp *= t;
          }
        }
      }
      dist_sum = 0.0;
      time_sum = 0.0;
    }
    time_sum += -dt + (T - t);  // "make sure the dt is correct for the next segment"
  }
  *cost = J;
  if (collision) *collision = is_collision ? 1 : 0;
  if (n_evaluated) *n_evaluated = evaluated;
  if (!grad) return;

  // L_pp^T: A(T_i)^-T = S(T) A(1)^-T diag(T^-j) per (segment, axis), in place
  const double* A1 = kA1inv + MTG_A1INV_OFF(N);
  for (int i = 0; i < K; ++i) {
    const double T = times[i], tinv = 1.0 / T;
    double s[6], u[12];
    s[0] = 1.0;
    for (int k = 1; k < h; ++k) s[k] = s[k - 1] * T;
    for (int k = 0; k < D; ++k) {
      double* acc = w.acc.data() + ((size_t)i * D + k) * N;
      double tp = 1.0;
      for (int j = 0; j < N; ++j) {
        u[j] = acc[j] * tp;
        tp *= tinv;
      }
      for (int q = 0; q < N; ++q) {
        double y = 0.0;
        for (int j = 0; j < N; ++j) y += A1[j * N + q] * u[j];
        acc[q] = s[q % h] * y;
      }
    }
  }
  const unsigned hm = (1u << h) - 1u;
  for (int k = 0; k < D; ++k) {
    double* g = grad + (size_t)k * V * h;
    int idx = 0;
    for (int v = 0; v <= K; ++v) {
      const unsigned mv = mask[v] & hm;
      for (int q = 0; q < h; ++q) {
        if ((mv >> q) & 1u) continue;
        const double bot = v > 0 ? w.acc[((size_t)(v - 1) * D + k) * N + h + q] : 0.0;
        const double top = v < K ? w.acc[((size_t)v * D + k) * N + q] : 0.0;
        g[idx++] = bot + top;
      }
    }
  }
}

int run(int N, int D, int K, int64_t batch, const double* vertex_values, const uint8_t* fixed_mask, const double* times,
        const double* coeff_times, const mtg_sdf_grid* grid, const mtg_collision_params* params, double* cost_out,
        double* grad_out, uint8_t* collision_out, int32_t* n_evaluated_out, int32_t* status, int threads) {
  if (N < 6 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D != 3) return MTG_ERR_INVALID_ARGUMENT;
  if (K < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (!grid || !params) return MTG_ERR_INVALID_ARGUMENT;
  if (!(params->coll_check_time_increment > 0.0) || !(params->map_resolution >= 0.0) || !(grid->resolution > 0.0) ||
      grid->nx < 1 || grid->ny < 1 || grid->nz < 1)
    return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !cost_out || !grid->distance || (grad_out && !fixed_mask)) return MTG_ERR_INVALID_ARGUMENT;
  const mtg::CollisionMap map{grid->distance, grid->nx, grid->ny, grid->nz,
                              {grid->origin[0], grid->origin[1], grid->origin[2]}, grid->resolution, grid->oob_distance};
  const mtg::CollisionPot pot{params->map_resolution, params->epsilon, params->robot_radius, params->coll_pot_multiplier,
                              {params->min_bound[0], params->min_bound[1], params->min_bound[2]},
                              {params->max_bound[0], params->max_bound[1], params->max_bound[2]},
                              params->use_continuous_distance ? 1 : 0};
  const double dt = params->coll_check_time_increment;
  const int h = N / 2, V = K + 1;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    Work w;
    for (int64_t b = b0; b < b1; ++b)
      one(N, K, vertex_values + b * (int64_t)V * h * D, fixed_mask ? fixed_mask + b * V : nullptr, times + b * K,
          coeff_times ? coeff_times + b * K : nullptr, map, pot, dt, cost_out + b,
          grad_out ? grad_out + b * (int64_t)D * V * h : nullptr, collision_out ? collision_out + b : nullptr,
          n_evaluated_out ? n_evaluated_out + b : nullptr, status ? status + b : nullptr, w);
  });
  return MTG_OK;
}

}  // namespace

extern "C" int mtg_host_collision_cost_batch(int N, int D, int K, int64_t batch, const double* vertex_values,
                                             const uint8_t* fixed_mask, const double* times, const mtg_sdf_grid* grid,
                                             const mtg_collision_params* params, double* cost_out, double* grad_out,
                                             uint8_t* collision_out, int32_t* n_evaluated_out, int32_t* status,
                                             int threads) {
  return run(N, D, K, batch, vertex_values, fixed_mask, times, nullptr, grid, params, cost_out, grad_out, collision_out,
             n_evaluated_out, status, threads);
}

// Host path of mtg_collision_cost_ragged_batch: the same per-trajectory code on each trajectory's blocks
// of the CSR arrays (vertices and mask at so[b] + b, times at so[b], the gradient block [3][V_b h] at
// double offset 3 h (so[b] + b)), threaded over trajectories.
extern "C" int mtg_host_collision_cost_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                                    const double* vertex_values, const uint8_t* fixed_mask,
                                                    const double* times, const mtg_sdf_grid* grid,
                                                    const mtg_collision_params* params, double* cost_out,
                                                    double* grad_out, uint8_t* collision_out, int32_t* n_evaluated_out,
                                                    int32_t* status, int threads) {
  if (N < 6 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D != 3) return MTG_ERR_INVALID_ARGUMENT;
  if (batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (!grid || !params) return MTG_ERR_INVALID_ARGUMENT;
  if (!(params->coll_check_time_increment > 0.0) || !(params->map_resolution >= 0.0) || !(grid->resolution > 0.0) ||
      grid->nx < 1 || grid->ny < 1 || grid->nz < 1)
    return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!seg_count) return MTG_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> so((size_t)batch + 1, 0);
  for (int64_t b = 0; b < batch; ++b) {
    if (seg_count[b] < 1) return MTG_ERR_SIZE_MISMATCH;
    so[(size_t)b + 1] = so[(size_t)b] + seg_count[b];
  }
  if (!vertex_values || !times || !cost_out || !grid->distance || (grad_out && !fixed_mask)) return MTG_ERR_INVALID_ARGUMENT;
  const mtg::CollisionMap map{grid->distance, grid->nx, grid->ny, grid->nz,
                              {grid->origin[0], grid->origin[1], grid->origin[2]}, grid->resolution, grid->oob_distance};
  const mtg::CollisionPot pot{params->map_resolution, params->epsilon, params->robot_radius, params->coll_pot_multiplier,
                              {params->min_bound[0], params->min_bound[1], params->min_bound[2]},
                              {params->max_bound[0], params->max_bound[1], params->max_bound[2]},
                              params->use_continuous_distance ? 1 : 0};
  const double dt = params->coll_check_time_increment;
  const int h = N / 2;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    Work w;
    for (int64_t b = b0; b < b1; ++b) {
      const int64_t s0 = so[(size_t)b], v0 = s0 + b;
      one(N, seg_count[b], vertex_values + v0 * h * D, fixed_mask ? fixed_mask + v0 : nullptr, times + s0, nullptr, map,
          pot, dt, cost_out + b, grad_out ? grad_out + v0 * D * h : nullptr, collision_out ? collision_out + b : nullptr,
          n_evaluated_out ? n_evaluated_out + b : nullptr, status ? status + b : nullptr, w);
    }
  });
  return MTG_OK;
}

int mtg::host_collision_cost_coeff_times(int N, int D, int K, int64_t batch, const double* vertex_values,
                                         const double* times, const double* coeff_times, const mtg_sdf_grid* grid,
                                         const mtg_collision_params* params, double* cost_out, uint8_t* collision_out,
                                         int32_t* n_evaluated_out, int32_t* status, int threads) {
  return run(N, D, K, batch, vertex_values, nullptr, times, coeff_times, grid, params, cost_out, nullptr, collision_out,
             n_evaluated_out, status, threads);
}
