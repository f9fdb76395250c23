// test_evaluate_range_ragged.cpp -- BatchPolynomialOptimization<10>::evaluateRangeRaggedCounts and
// evaluateRangeRagged on five trajectories of 3, 1, 4, 1 and 3 segments in one CSR batch, against
// Trajectory::evaluateRange called per trajectory on the host policy (the reference's sequential
// clock), bit for bit: counts, samples and sampling times.  Needs a GPU.
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

int main() {
  mtg::setExecutionPolicy(mtg::ExecutionPolicy::kHost);  // (Trajectory::evaluateRange on the calling thread)
  constexpr int N = 10;
  const int B = 5, D = 3, derivative = 1;
  const double t_start = 0.25, t_end = 4.0, dt = 0.01;  // t_end cuts the long trajectories mid-segment
  const std::vector<int32_t> seg = {3, 1, 4, 1, 3};
  std::mt19937_64 rng(20241021);
  std::uniform_real_distribution<double> uc(-2.0, 2.0), ut(0.3, 2.5);
  std::vector<mtg::Trajectory> traj(B);
  std::vector<double> coeffs, times;
  for (int b = 0; b < B; ++b) {
    mtg::Segment::Vector segs;
    for (int i = 0; i < seg[b]; ++i) {
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
  }
  mtg::BatchPolynomialOptimization<N> opt(D, 7, 4);  // (its segment count is not used)
  std::vector<int64_t> counts(B, -1), offsets(B, 0);
  opt.evaluateRangeRaggedCounts(B, seg.data(), times.data(), t_start, t_end, dt, counts.data());
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    offsets[b] = total;
    total += counts[b];
  }
  std::vector<double> out((size_t)total * D, -1.0), st((size_t)total, -1.0);
  opt.evaluateRangeRagged(B, seg.data(), coeffs.data(), times.data(), t_start, t_end, dt, derivative, counts.data(),
                          offsets.data(), out.data(), st.data());
  for (int b = 0; b < B; ++b) {
    std::vector<mtg::VectorXd> want;
    std::vector<double> want_t;
    traj[b].evaluateRange(t_start, t_end, dt, derivative, &want, &want_t);
    if (want.empty()) std::printf("trajectory %d has no sample: the case is too weak\n", b), ++fails;
    if (counts[b] != (int64_t)want.size()) {
      std::printf("counts[%d] = %lld, want %zu\n", b, (long long)counts[b], want.size()), ++fails;
      continue;
    }
    for (size_t n = 0; n < want.size(); ++n) {
      const size_t row = (size_t)offsets[b] + n;
      if (bits(st[row]) != bits(want_t[n]))
        std::printf("b %d sample %zu time: %.17g, want %.17g\n", b, n, st[row], want_t[n]), ++fails;
      for (int d = 0; d < D; ++d)
        if (bits(out[row * D + d]) != bits(want[n][d]))
          std::printf("b %d sample %zu dim %d: %.17g, want %.17g\n", b, n, d, out[row * D + d], want[n][d]), ++fails;
      if (fails > 20) break;
    }
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
