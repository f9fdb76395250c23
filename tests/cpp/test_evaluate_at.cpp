// test_evaluate_at.cpp -- the free evaluateAt<10> of batch_polynomial_optimization.h against
// Trajectory::evaluate called in a loop, bit for bit: 3 trajectories x 9 query times that include a
// vertex time, the end time and one beyond the end.  "host" runs the host policy, "device" the kernels
// (ExecutionPolicy::kDevice) and the batch object's member.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"
#include "mav_trajectory_generation/trajectory.h"

namespace mtg = mav_trajectory_generation;

static int fails = 0;

static uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, sizeof(u));
  return u;
}

int main(int argc, char** argv) {
  const bool device = argc > 1 && !std::strcmp(argv[1], "device");
  mtg::setExecutionPolicy(device ? mtg::ExecutionPolicy::kDevice : mtg::ExecutionPolicy::kHost);
  constexpr int N = 10;
  const int B = 3, D = 3, K = 4, M = 9, nd = 3;
  std::mt19937_64 rng(20240521);
  std::uniform_real_distribution<double> uc(-2.0, 2.0), ut(0.3, 2.5), u01(0.0, 1.0);
  std::vector<mtg::Trajectory> traj(B);
  std::vector<double> coeffs, times, tq((size_t)B * M);
  for (int b = 0; b < B; ++b) {
    mtg::Segment::Vector segs;
    for (int i = 0; i < K; ++i) {
      mtg::Segment s(N, D);
      s.setTime(ut(rng));
      for (int d = 0; d < D; ++d) {
        mtg::VectorXd c(N);
        for (int j = 0; j < N; ++j) c[j] = uc(rng);
        s[d].setCoefficients(c);
      }
      segs.push_back(s);
    }
    traj[b].setSegments(segs);
    std::vector<double> c, t;
    traj[b].pack(&c, &t);
    coeffs.insert(coeffs.end(), c.begin(), c.end());
    times.insert(times.end(), t.begin(), t.end());
    // the accumulated times as Trajectory::evaluate forms them
    double acc = 0.0, vertex2 = 0.0;
    for (int i = 0; i < K; ++i) {
      acc += t[i];
      if (i == 1) vertex2 = acc;
    }
    double* q = &tq[(size_t)b * M];
    q[0] = 0.0;
    q[1] = vertex2;                        // a vertex time: the segment to its right
    q[2] = acc;                            // the end time: the last segment at its end
    q[3] = acc + 0.5;                      // beyond the end: zeros
    q[4] = std::nextafter(acc, 0.0);
    q[5] = std::nextafter(vertex2, 0.0);
    for (int m = 6; m < M; ++m) q[m] = acc * u01(rng);
  }
  std::vector<double> out((size_t)B * M * nd * D, -1.0);
  std::vector<uint8_t> in_range((size_t)B * M, 7);
  std::vector<int32_t> status(B, -1);
  mtg::evaluateAt<N>(D, K, B, coeffs.data(), times.data(), tq.data(), M, M, 0, nd, out.data(), in_range.data(),
                     status.data());
  std::vector<double> out2(out.size(), -1.0);
  if (device) {
    mtg::BatchPolynomialOptimization<N> opt(D, K, 4);
    opt.evaluateAt(B, coeffs.data(), times.data(), tq.data(), M, M, 0, nd, out2.data());
  }
  for (int b = 0; b < B; ++b) {
    if (status[b] != MTG_TRAJ_OK) std::printf("status[%d] = %d\n", b, status[b]), ++fails;
    for (int m = 0; m < M; ++m) {
      const double t = tq[(size_t)b * M + m];
      const int want_in = m == 3 ? 0 : 1;
      if (in_range[(size_t)b * M + m] != want_in) std::printf("in_range[%d][%d] = %d\n", b, m, in_range[(size_t)b * M + m]), ++fails;
      for (int k = 0; k < nd; ++k) {
        const mtg::VectorXd want = traj[b].evaluate(t, k);  // (m == 3 prints the reference's error line)
        for (int d = 0; d < D; ++d) {
          const size_t at = (((size_t)b * M + m) * nd + k) * D + d;
          if (bits(out[at]) != bits(want[d]))
            std::printf("b %d m %d order %d dim %d: %.17g, want %.17g\n", b, m, k, d, out[at], want[d]), ++fails;
          if (device && bits(out2[at]) != bits(want[d]))
            std::printf("member: b %d m %d order %d dim %d: %.17g, want %.17g\n", b, m, k, d, out2[at], want[d]), ++fails;
        }
      }
    }
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
