// test_soft_constraint_api.cpp -- softConstraintCost<N> of batch_polynomial_optimization.h on the host
// policy ("host", the default) or through the GPU ("device"): the known answer of a straight,
// constant-velocity segment in one dimension, computed by hand, and the gradient against the central
// difference of two cost-only calls.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"

namespace mtg = mav_trajectory_generation;

int main(int argc, char** argv) {
  const bool device = argc > 1 && !std::strcmp(argv[1], "device");
  mtg::setExecutionPolicy(device ? mtg::ExecutionPolicy::kDevice : mtg::ExecutionPolicy::kHost);
  // one segment, N = 6, D = 1: p(t) = -1 + 2 t on [0, 2]
  const int K = 1, h = 3, D = 1;
  const double T = 2.0;
  std::vector<double> x((size_t)(K + 1) * h * D, 0.0);
  x[0 * h + 0] = -1.0, x[0 * h + 1] = 2.0;
  x[1 * h + 0] = 3.0, x[1 * h + 1] = 2.0;
  const uint8_t mask[2] = {7, 5};  // free: the velocity of vertex 1
  mtg_soft_constraint_params p{};
  p.n_constraints = 2;
  p.derivative[0] = 1, p.limit[0] = 1.6;  // |v| = 2 everywhere: the first candidate, t = 0, is kept
  p.derivative[1] = 0, p.limit[1] = 2.5;  // |p| is largest at t = T = 2 (value 3): the end candidate
  p.weight = 10.0;
  p.maximum_cost = 1e12;
  p.increment = 0.05;

  int fails = 0;
  double cost = -1.0, grad[6] = {9, 9, 9, 9, 9, 9};
  mtg_extremum mx[2];
  int32_t status = -1;
  mtg::softConstraintCost<6>(D, K, 1, x.data(), mask, &T, p, &cost, grad, mx, &status);
  const double want = std::exp(10.0 * (2.0 - 1.6) / 1.6) + std::exp(10.0 * (3.0 - 2.5) / 2.5);
  if (!(std::fabs(cost - want) <= 1e-12 * want)) std::printf("cost %.17g, want %.17g\n", cost, want), ++fails;
  if (status != MTG_TRAJ_OK) std::printf("status %d\n", status), ++fails;
  if (!(std::fabs(mx[0].value - 2.0) <= 1e-13) || mx[0].time != 0.0 || mx[0].segment != 0)
    std::printf("velocity maximum (%g, %.17g, %d), want (0, 2, 0)\n", mx[0].time, mx[0].value, mx[0].segment), ++fails;
  if (!(std::fabs(mx[1].value - 3.0) <= 1e-13) || mx[1].time != T || mx[1].segment != 0)
    std::printf("position maximum (%g, %.17g, %d), want (2, 3, 0)\n", mx[1].time, mx[1].value, mx[1].segment), ++fails;

  // the gradient entry of the one free derivative against two cost-only calls; the rest is 0
  double cl = 0.0, cr = 0.0, c0 = 0.0;
  std::vector<double> xp = x;
  xp[1 * h + 1] = 2.0 - p.increment;
  mtg::softConstraintCost<6>(D, K, 1, xp.data(), nullptr, &T, p, &cl);
  xp[1 * h + 1] = 2.0 + p.increment;
  mtg::softConstraintCost<6>(D, K, 1, xp.data(), nullptr, &T, p, &cr);
  mtg::softConstraintCost<6>(D, K, 1, x.data(), nullptr, &T, p, &c0);
  const double gwant = (cr - cl) / (2.0 * p.increment);
  if (!(std::fabs(grad[0] - gwant) <= 1e-9 * (cl + cr) / (2.0 * p.increment)) || !(std::fabs(gwant) > 1.0))
    std::printf("grad %.17g, want %.17g\n", grad[0], gwant), ++fails;
  for (int e = 1; e < 6; ++e)
    if (grad[e] != 0.0) std::printf("grad[%d] = %g, want 0\n", e, grad[e]), ++fails;
  if (std::memcmp(&c0, &cost, sizeof c0)) std::printf("cost without gradient %.17g != with %.17g\n", c0, cost), ++fails;

#ifdef MTG_CPP_THROW
  bool threw = false;
  try {
    p.limit[1] = 0.0;
    mtg::softConstraintCost<6>(D, K, 1, x.data(), nullptr, &T, p, &cost);
  } catch (const mtg::Error& e) {
    threw = e.code == MTG_ERR_INVALID_ARGUMENT;
  }
  if (!threw) std::printf("limit = 0 did not raise MTG_ERR_INVALID_ARGUMENT\n"), ++fails;
#endif
  if (fails) return 1;
  std::printf("all checks passed\n");
  return 0;
}
