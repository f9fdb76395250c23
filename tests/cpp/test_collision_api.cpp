// test_collision_api.cpp -- collisionCost<N> of batch_polynomial_optimization.h on the host policy:
// the known answer of a straight, constant-velocity segment flown parallel to a planar distance
// field (distance = z), computed by hand.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"

namespace mtg = mav_trajectory_generation;

int main() {
  mtg::setExecutionPolicy(mtg::ExecutionPolicy::kHost);
  // planar field distance = z on a 64^3 grid, origin -8, resolution 0.25 (cell centres exact in float)
  const int n = 64;
  std::vector<float> field((size_t)n * n * n);
  for (int ix = 0; ix < n; ++ix)
    for (int iy = 0; iy < n; ++iy)
      for (int iz = 0; iz < n; ++iz) field[((size_t)ix * n + iy) * n + iz] = (float)(-8.0 + (iz + 0.5) * 0.25);
  mtg_sdf_grid grid{field.data(), n, n, n, {-8.0, -8.0, -8.0}, 0.25, 100.0};
  mtg_collision_params p{};
  p.coll_check_time_increment = 0.125;
  p.map_resolution = 0.0;
  p.epsilon = 0.5;
  p.robot_radius = 0.125;
  p.coll_pot_multiplier = 1.0;
  for (int k = 0; k < 3; ++k) p.min_bound[k] = -8.0, p.max_bound[k] = 8.0;
  p.use_continuous_distance = 0;

  // one segment, N = 6: position x0 + v t along x at height z0 = 0.375 (a cell centre), T = 1
  const int K = 1, h = 3;
  const double v = 2.0, T = 1.0, z0 = 0.375;
  std::vector<double> x((size_t)(K + 1) * h * 3, 0.0);
  const double start[3] = {-1.0, 0.125, z0}, end[3] = {-1.0 + v * T, 0.125, z0};
  for (int d = 0; d < 3; ++d) x[(0 * h + 0) * 3 + d] = start[d], x[(1 * h + 0) * 3 + d] = end[d];
  x[(0 * h + 1) * 3 + 0] = v;
  x[(1 * h + 1) * 3 + 0] = v;
  double cost = -1.0;
  uint8_t hit = 9;
  int32_t evaluated = -1, status = -1;
  mtg::collisionCost<6>(K, 1, x.data(), nullptr, &T, grid, p, &cost, nullptr, &hit, &evaluated, &status);

  // by hand: samples at t = 0, 0.125, ..., 0.875; the first is skipped, the other seven each carry
  // time_sum = dt; d = z0 - radius = 0.25 <= epsilon: c = 0.5 / 0.5 * (0.25 - 0.5)^2 = 0.0625
  const double want = 7.0 * 0.0625 * v * 0.125;
  int fails = 0;
  if (!(std::fabs(cost - want) <= 1e-12 * want)) std::printf("cost %.17g, want %.17g\n", cost, want), ++fails;
  if (evaluated != 7) std::printf("n_evaluated %d, want 7\n", evaluated), ++fails;
  if (hit != 0) std::printf("collision flag %d, want 0\n", (int)hit), ++fails;
  if (status != MTG_TRAJ_OK) std::printf("status %d\n", status), ++fails;

  // inside the obstacle: z0 below the robot radius sets the flag
  for (int v2 = 0; v2 < 2; ++v2) x[(v2 * h + 0) * 3 + 2] = -0.125;
  mtg::collisionCost<6>(K, 1, x.data(), nullptr, &T, grid, p, &cost, nullptr, &hit, &evaluated, &status);
  const double want2 = 7.0 * (1.0 * 0.25 + 0.25) * v * 0.125;  // d = -0.125 - 0.125: multiplier * 0.25 + epsilon / 2
  if (!(std::fabs(cost - want2) <= 1e-12 * want2)) std::printf("cost %.17g, want %.17g\n", cost, want2), ++fails;
  if (hit != 1) std::printf("collision flag %d, want 1\n", (int)hit), ++fails;

#ifdef MTG_CPP_THROW
  bool threw = false;
  try {
    p.coll_check_time_increment = 0.0;
    mtg::collisionCost<6>(K, 1, x.data(), nullptr, &T, grid, p, &cost);
  } catch (const mtg::Error& e) {
    threw = e.code == MTG_ERR_INVALID_ARGUMENT;
  }
  if (!threw) std::printf("dt = 0 did not raise MTG_ERR_INVALID_ARGUMENT\n"), ++fails;
#endif
  if (fails) return 1;
  std::printf("all checks passed\n");
  return 0;
}
