// BatchPolynomialOptimization<N>::solveRagged (mtg_solve_linear_ragged_batch) of the C++ drop-in: both
// overloads, from vertex lists of 3, 11 and 12 vertices, against three PolynomialOptimization<10>
// drop-in solves.  Built by CMake (target test_ragged) or directly by tests/test_gpu_ragged.py.
//
//   test_ragged device   needs a HIP device (the class creates a context)
// Exit status 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"
#include "mav_trajectory_generation/polynomial_optimization_linear.h"

using namespace mav_trajectory_generation;

static int g_fail = 0;
#define EXPECT(cond, ...)                                       \
  do {                                                          \
    if (!(cond)) {                                              \
      ++g_fail;                                                 \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fprintf(stderr, "\n");                               \
    }                                                           \
  } while (0)

static int run_device() {
  constexpr int N = 10, D = 3, r = 4;
  setExecutionPolicy(ExecutionPolicy::kDevice);  // the single problems go through the GPU too
  const int segments[3] = {2, 10, 11};           // 3, 11 and 12 vertices
  const VectorXd pmin = VectorXd::Constant(D, -10.0), pmax = VectorXd::Constant(D, 10.0);
  std::vector<Vertex::Vector> problems;
  std::vector<std::vector<double>> times;
  for (int p = 0; p < 3; ++p) {
    problems.push_back(createRandomVertices(4, segments[p], pmin, pmax, 2000 + p));
    times.push_back(estimateSegmentTimes(problems.back(), 3.0, 5.0));
    EXPECT((int)problems.back().size() == segments[p] + 1, "vertex count");
  }
  // the object's segment count plays no part in solveRagged
  BatchPolynomialOptimization<N> batch(D, 1, r);
  std::vector<double> coeffs, cost;
  std::vector<int64_t> so;
  std::vector<int32_t> status;
  batch.solveRagged(problems, times, &coeffs, &so, &cost, &status);
  EXPECT(so.size() == 4 && so[0] == 0 && so[1] == 2 && so[2] == 12 && so[3] == 23, "segment offsets");
  EXPECT(coeffs.size() == (size_t)23 * D * N && cost.size() == 3 && status.size() == 3, "output sizes");
  for (int p = 0; p < 3 && so.size() == 4; ++p) {
    PolynomialOptimization<N> opt(D);
    opt.setupFromVertices(problems[p], times[p], r);
    opt.solveLinear();
    Segment::Vector segs;
    opt.getSegments(&segs);
    EXPECT(status[p] == 0, "status of problem %d: %d", p, status[p]);
    // the tolerance of tests/cpp/test_cpp_api.cpp between the batched entry and the drop-in on the
    // device: the same coefficients, and the cost to 1e-7 (computeCost forms Q with pow())
    for (int i = 0; i < segments[p]; ++i)
      for (int d = 0; d < D; ++d) {
        const VectorXd c = segs[i][d].getCoefficients();
        for (int j = 0; j < N; ++j)
          EXPECT(c[j] == coeffs[((size_t)(so[p] + i) * D + d) * N + j], "problem %d seg %d dim %d c[%d]", p, i, d, j);
      }
    const double ref = opt.computeCost();
    EXPECT(std::fabs(cost[p] - ref) <= 1e-7 * std::fmax(ref, 1e-12), "cost of problem %d: %.17g vs %.17g", p, cost[p],
           ref);
  }
  // the pointer overload on the same problems packed by hand: the same bytes
  const int h = N / 2;
  const int32_t seg[3] = {2, 10, 11};
  std::vector<double> vals((size_t)26 * h * D), t(23), coeffs2((size_t)23 * D * N), cost2(3);
  std::vector<uint8_t> mask(26);
  std::vector<int32_t> status2(3);
  for (int p = 0; p < 3; ++p) {
    const size_t v0 = (size_t)(so.size() == 4 ? so[p] : 0) + p;
    packVertices(problems[p], N, D, vals.data() + v0 * h * D, mask.data() + v0);
    for (int i = 0; i < seg[p]; ++i) t[v0 - p + i] = times[p][i];
  }
  batch.solveRagged(3, seg, vals.data(), mask.data(), t.data(), coeffs2.data(), cost2.data(), status2.data());
  EXPECT(coeffs2 == coeffs && cost2 == cost && status2 == status, "pointer overload vs vertex-list overload");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode != "device") {
    std::fprintf(stderr, "usage: test_ragged device   (needs a HIP device)\n");
    return 2;
  }
  run_device();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("test_ragged (%s): all checks passed\n", mode.c_str());
  return 0;
}
