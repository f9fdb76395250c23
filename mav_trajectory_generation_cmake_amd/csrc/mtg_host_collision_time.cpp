// mtg_host_collision_time.cpp -- host (CPU) path of mtg_collision_time_gradient_batch: the collision
// part dJc_dt of the reference's getCostAndGradientTime
// (polynomial_optimization_nonlinear_impl.h:2155-2243) written literally.  Per trajectory the
// coefficients are formed once from the unperturbed times (the reference's L_ is not recomputed by
// updateSegmentTimes), then for every segment n and side (smaller first) one COMPLETE walk of
// getCostAndGradientCollision's loop (:1563-1709, no gradient) over the perturbed times: 2K walks.
// The per-position part is mtg_collision_common.h, shared with the kernels.  Plain C++ (no HIP).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <thread>
#include <vector>

#include "mtg.h"
#include "mtg_collision_common.h"
#include "mtg_host_threads.h"

namespace {

// the loop of mtg_host_collision.cpp without the gradient, over segment times tp
double walk(int N, int K, const double* coeffs, const double* tp, const mtg::CollisionMap& map,
            const mtg::CollisionPot& pot, double dt, int32_t* evaluated_out) {
  double J = 0.0;
  int32_t evaluated = 0;
  double prev[3] = {0.0, 0.0, 0.0};
  double time_sum = -1.0, dist_sum = 0.0;
  for (int i = 0; i < K; ++i) {
    const double T = tp[i];
    double t;
    for (t = 0.0; t < T; t += dt) {
      double pos[3], vel[3];
      for (int k = 0; k < 3; ++k) {
        const double* c = coeffs + ((size_t)i * 3 + k) * N;
        double p = c[N - 1], v = (double)(N - 1) * c[N - 1];
        for (int n = N - 2; n >= 0; --n) p = p * t + c[n];
        for (int n = N - 2; n >= 1; --n) v = v * t + (double)n * c[n];
        pos[k] = p;
        vel[k] = v;
      }
      if (time_sum < 0) {  // numerical integration: skip the first entry
        time_sum = 0.0;
        for (int k = 0; k < 3; ++k) prev[k] = pos[k];
        continue;
      }
      time_sum += dt;
      const double dx = pos[0] - prev[0], dy = pos[1] - prev[1], dz = pos[2] - prev[2];
      dist_sum += std::sqrt(dx * dx + dy * dy + dz * dz);
      for (int k = 0; k < 3; ++k) prev[k] = pos[k];
      if (dist_sum < pot.increment) continue;
      double gc[3];
      bool pos_collision;
      const double c = mtg::collision_potential_at(map, pot, pos, false, gc, pos_collision);
      ++evaluated;
      const double vn = std::sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]);
      J += c * vn * time_sum;
      dist_sum = 0.0;
      time_sum = 0.0;
    }
    time_sum += -dt + (T - t);
  }
  *evaluated_out = evaluated;
  return J;
}

struct Work {
  std::vector<double> coeffs;  // [K][3][N], from the unperturbed times
  std::vector<double> tp;      // [K] perturbed times
};

void one(int N, int K, const double* values, const double* times, const mtg::CollisionMap& map,
         const mtg::CollisionPot& pot, double dt, double inc, double* grad_t, double* side_cost, int32_t* side_evaluated,
         int32_t* status, Work& w) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  bool bad = false;
  for (int i = 0; i < K; ++i) bad |= mtg::collision_time_bad(times[i], inc, dt);
  if (status) *status = bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
  if (bad) {
    for (int n = 0; n < K; ++n) {
      grad_t[n] = nan;
      for (int s = 0; s < 2; ++s) {
        if (side_cost) side_cost[2 * n + s] = nan;
        if (side_evaluated) side_evaluated[2 * n + s] = 0;
      }
    }
    return;
  }
  w.coeffs.resize((size_t)K * 3 * N);
  mtg_host_coefficients_from_vertices_batch(N, 3, K, 1, values, times, w.coeffs.data(), 1);
  w.tp.assign(times, times + K);
  for (int n = 0; n < K; ++n) {
    double J[2] = {nan, nan};
    int32_t ev[2] = {0, 0};
    const bool clamp = times[n] <= mtg::kCollisionTimeClamp;
    if (clamp || times[n] - inc > 0.0) {  // otherwise the reference CHECK-fails in updateSegmentTimes
      for (int s = 0; s < 2; ++s) {
        w.tp[n] = mtg::collision_time_perturbed(times[n], inc, s);
        J[s] = walk(N, K, w.coeffs.data(), w.tp.data(), map, pot, dt, &ev[s]);
      }
      w.tp[n] = times[n];
    }
    grad_t[n] = (J[1] - J[0]) / (2.0 * inc);
    for (int s = 0; s < 2; ++s) {
      if (side_cost) side_cost[2 * n + s] = J[s];
      if (side_evaluated) side_evaluated[2 * n + s] = ev[s];
    }
  }
}

}  // namespace

extern "C" int mtg_host_collision_time_gradient_batch(int N, int D, int K, int64_t batch, const double* vertex_values,
                                                      const double* times, const mtg_sdf_grid* grid,
                                                      const mtg_collision_params* params, double increment_time,
                                                      double* grad_t_out, double* side_cost_out,
                                                      int32_t* side_evaluated_out, int32_t* status, int threads) {
  if (N < 6 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  if (D != 3) return MTG_ERR_INVALID_ARGUMENT;
  if (K < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (!grid || !params) return MTG_ERR_INVALID_ARGUMENT;
  if (!(params->coll_check_time_increment > 0.0) || !(params->map_resolution >= 0.0) || !(grid->resolution > 0.0) ||
      grid->nx < 1 || grid->ny < 1 || grid->nz < 1)
    return MTG_ERR_INVALID_ARGUMENT;
  if (!(increment_time > 0.0 && increment_time <= DBL_MAX)) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!vertex_values || !times || !grad_t_out || !grid->distance) return MTG_ERR_INVALID_ARGUMENT;
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
      one(N, K, vertex_values + b * (int64_t)V * h * 3, times + b * K, map, pot, dt, increment_time, grad_t_out + b * K,
          side_cost_out ? side_cost_out + b * 2 * K : nullptr, side_evaluated_out ? side_evaluated_out + b * 2 * K : nullptr,
          status ? status + b : nullptr, w);
  });
  return MTG_OK;
}
