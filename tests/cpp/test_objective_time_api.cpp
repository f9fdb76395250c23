// test_objective_time_api.cpp -- objectiveTime<N> of batch_polynomial_optimization.h on the host policy
// for one trajectory of N = 6, K = 1, D = 3 (tests/_objective_cases.py's `k1`), read from a file of
// doubles that tests/test_objective_time_host.py writes: values [2][3][3], the time, x of objective 4
// [x_stride], then weight, maximum_cost, increment and the two limits of the soft constraints.
// Arguments: file mask0 mask1 x_stride derivative0 derivative1.  Prints the cost of objective 3 (no
// collision term) and of objective 4 as hexadecimal doubles; the Python test compares the bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"

namespace mtg = mav_trajectory_generation;

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  mtg::setExecutionPolicy(mtg::ExecutionPolicy::kHost);
  const int N = 6, K = 1, D = 3, h = N / 2;
  const int64_t stride = std::atoll(argv[4]);
  const size_t want = (size_t)(K + 1) * h * D + K + (size_t)stride + 5;
  std::vector<double> in(want);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), want, f) != want) return 3;
  std::fclose(f);
  const double* values = in.data();
  const double* time = values + (K + 1) * h * D;
  const double* x4 = time + K;
  const double* sp = x4 + stride;
  const uint8_t mask[2] = {(uint8_t)std::atoi(argv[2]), (uint8_t)std::atoi(argv[3])};
  mtg_soft_constraint_params soft{};
  soft.n_constraints = 2;
  soft.derivative[0] = std::atoi(argv[5]);
  soft.derivative[1] = std::atoi(argv[6]);
  soft.weight = sp[0];
  soft.maximum_cost = sp[1];
  soft.increment = sp[2];
  soft.limit[0] = sp[3];
  soft.limit[1] = sp[4];
  mtg_objective_time_params p{};
  p.derivative_to_optimize = 2;
  p.time_penalty = 500.0;
  p.w_c = 0.0;
  p.use_soft_constraints = 1;
  double cost3 = 0.0, cost4 = 0.0;
  p.objective = MTG_OBJECTIVE_TIME;
  mtg::objectiveTime<N>(D, K, 1, values, mask, time, K, p, nullptr, nullptr, nullptr, &soft, &cost3);
  p.objective = MTG_OBJECTIVE_TIME_AND_CONSTRAINTS;
  mtg::objectiveTime<N>(D, K, 1, values, mask, x4, stride, p, nullptr, nullptr, nullptr, &soft, &cost4);
  std::printf("%a %a\n", cost3, cost4);
  return 0;
}
