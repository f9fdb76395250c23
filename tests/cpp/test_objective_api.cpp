// test_objective_api.cpp -- objective<N> and BatchPolynomialOptimization<N>::objective of
// batch_polynomial_optimization.h against the C ABI (mtg_host_objective_batch / mtg_objective_batch),
// byte for byte, and against a hand-computed answer: the straight, constant-velocity flight parallel
// to a planar distance field of test_collision_time_api.cpp, whose derivative cost is zero.  "host"
// runs the host policy, "device" the kernels (ExecutionPolicy::kDevice and the batch object).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"

namespace mtg = mav_trajectory_generation;

static int fails = 0;

static void near(const char* what, double got, double want, double tol) {
  if (!(std::fabs(got - want) <= tol)) std::printf("%s: %.17g, want %.17g\n", what, got, want), ++fails;
}

int main(int argc, char** argv) {
  const bool device = argc > 1 && !std::strcmp(argv[1], "device");
  mtg::setExecutionPolicy(device ? mtg::ExecutionPolicy::kDevice : mtg::ExecutionPolicy::kHost);
  const int n = 64;
  std::vector<float> field((size_t)n * n * n);
  for (int ix = 0; ix < n; ++ix)
    for (int iy = 0; iy < n; ++iy)
      for (int iz = 0; iz < n; ++iz) field[((size_t)ix * n + iy) * n + iz] = (float)(-8.0 + (iz + 0.5) * 0.25);
  mtg_sdf_grid grid{field.data(), n, n, n, {-8.0, -8.0, -8.0}, 0.25, 100.0};
  mtg_collision_params cp{};
  cp.coll_check_time_increment = 0.125;
  cp.map_resolution = 0.0;
  cp.epsilon = 0.5;
  cp.robot_radius = 0.125;
  cp.coll_pot_multiplier = 1.0;
  for (int k = 0; k < 3; ++k) cp.min_bound[k] = -8.0, cp.max_bound[k] = 8.0;

  // two segments, N = 6: x = -1 + 2 t at y = 0.125, z = 0.375, T = (1, 0.0625).  The ends fix every
  // derivative, the interior vertex its position: velocity and acceleration there are free, n_free = 2.
  const int K = 2, h = 3, D = 3;
  const double T[2] = {1.0, 0.0625}, xs[3] = {-1.0, 1.0, 1.125};
  std::vector<double> values((size_t)(K + 1) * h * D, 0.0);
  for (int q = 0; q <= K; ++q) {
    values[(q * h + 0) * D + 0] = xs[q];
    values[(q * h + 0) * D + 1] = 0.125;
    values[(q * h + 0) * D + 2] = 0.375;
    values[(q * h + 1) * D + 0] = 2.0;
  }
  const uint8_t mask[3] = {7, 1, 7};
  const int64_t stride = 9;  // the row has 6 entries (objective 1) or 8 (objective 2)
  mtg_objective_params p{};
  p.derivative_to_optimize = 2;
  p.w_d = 0.1, p.w_c = 10.0, p.w_t = 1.0, p.w_sc = 1.0;
  p.increment_time = 0.25;
  p.use_soft_constraints = 0;

  // objective 1 by hand: J_d = 0 (no acceleration), J_c = 7 samples of c v dt with c = 0.0625
  // (test_collision_time_api.cpp), so cost = w_c J_c
  p.objective = MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION;
  const double x1[9] = {2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 99.0, 99.0, 99.0};  // (the padding is not read)
  double cost = -1.0, grad[9], w[4];
  uint8_t coll = 9;
  int32_t status = -1;
  mtg_objective_state state{};
  mtg::objective<6>(D, K, 1, values.data(), mask, T, x1, stride, p, &grid, &cp, nullptr, &cost, grad, w, &coll, &state,
                    nullptr, &status);
  const double Jc = 7.0 * 0.0625 * 2.0 * 0.125;
  near("objective 1 cost", cost, 10.0 * Jc, 1e-9);
  near("weighted collision cost", w[1], 10.0 * Jc, 1e-9);
  if (status != MTG_TRAJ_OK || coll != 0 || state.n_iterations != 1 || !state.iter0_done || state.total_cost_iter0 != cost)
    std::printf("objective 1: status %d, collision %d, state (%d, %d)\n", status, coll, state.n_iterations, state.iter0_done), ++fails;
  for (int j = 6; j < 9; ++j)
    if (grad[j] != 0.0 || std::signbit(grad[j])) std::printf("grad padding [%d] = %g\n", j, grad[j]), ++fails;

  // the wrapper against the C ABI, byte for byte, on objective 2 with a state carried over two calls
  p.objective = MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME;
  p.is_collision_safe = 1;
  p.is_coll_raise_first_iter = 1;
  p.add_coll_raise = 0.5;
  const double x2[9] = {1.0, 0.0625, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, -5.0};
  double costA[2], gradA[2][9], wA[2][4], costB[2], gradB[2][9], wB[2][4];
  uint8_t collA[2], collB[2];
  int32_t stA[2], stB[2];
  mtg_objective_state sA{}, sB{};
  mtg::BatchPolynomialOptimization<6>* opt = device ? new mtg::BatchPolynomialOptimization<6>(D, K, 2) : nullptr;
  for (int it = 0; it < 2; ++it) {
    mtg::objective<6>(D, K, 1, values.data(), mask, nullptr, x2, stride, p, &grid, &cp, nullptr, &costA[it], gradA[it],
                      wA[it], &collA[it], &sA, nullptr, &stA[it]);
    int rc;
    if (device)
      rc = mtg_objective_batch(opt->context(), 6, D, K, 1, values.data(), mask, nullptr, x2, stride, &p, &grid, &cp,
                               nullptr, &costB[it], gradB[it], wB[it], &collB[it], &sB, nullptr, &stB[it], 0);
    else
      rc = mtg_host_objective_batch(6, D, K, 1, values.data(), mask, nullptr, x2, stride, &p, &grid, &cp, nullptr,
                                    &costB[it], gradB[it], wB[it], &collB[it], &sB, nullptr, &stB[it], 1);
    if (rc != MTG_OK) std::printf("C ABI call failed: %d\n", rc), ++fails;
  }
  if (std::memcmp(costA, costB, sizeof costA) || std::memcmp(gradA, gradB, sizeof gradA) || std::memcmp(wA, wB, sizeof wA) ||
      std::memcmp(collA, collB, sizeof collA) || std::memcmp(stA, stB, sizeof stA) || std::memcmp(&sA, &sB, sizeof sA))
    std::printf("free function and C ABI differ\n"), ++fails;
  near("objective 2 cost", costA[0], 10.0 * Jc + 1.0625, 1e-9);
  near("time gradient of the floored segment", gradA[0][1], 1.0, 1e-12);  // T <= 0.1: both terms exactly 0, plus w_t
  if (sA.n_iterations != 2) std::printf("n_iterations = %d, want 2\n", sA.n_iterations), ++fails;
  if (device) {  // the batch object's member, with its own derivative_to_optimize
    double costC, gradC[9], wC[4];
    uint8_t collC;
    int32_t stC;
    mtg_objective_state sC{};
    mtg_objective_params q = p;
    q.derivative_to_optimize = 0;  // overwritten by the member
    opt->objective(1, values.data(), mask, nullptr, x2, stride, q, &grid, &cp, nullptr, &costC, gradC, wC, &collC, &sC,
                   nullptr, &stC);
    if (std::memcmp(&costC, &costA[0], sizeof costC) || std::memcmp(gradC, gradA[0], sizeof gradC) ||
        std::memcmp(wC, wA[0], sizeof wC))
      std::printf("member and free function differ\n"), ++fails;
    delete opt;
  }

#ifdef MTG_CPP_THROW
  {
    mtg_objective_params bad = p;
    bad.reserved = MTG_OBJECTIVE_USE_NUMERIC_GRAD;
    bool threw = false;
    try {
      mtg::objective<6>(D, K, 1, values.data(), mask, nullptr, x2, stride, bad, &grid, &cp, nullptr, &cost);
    } catch (const mtg::Error& e) {
      threw = e.code == MTG_ERR_INVALID_ARGUMENT;
    }
    if (!threw) std::printf("use_numeric_grad did not raise MTG_ERR_INVALID_ARGUMENT\n"), ++fails;
  }
#endif
  if (fails) return 1;
  std::printf("all checks passed\n");
  return 0;
}
