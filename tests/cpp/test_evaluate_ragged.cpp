// test_evaluate_ragged.cpp -- the free evaluateAtRagged<10> and minMaxMagnitudeRagged<10> of
// batch_polynomial_optimization.h on five trajectories of 3, 1, 4, 1 and 3 segments in one CSR batch
// (no K-group is one run of it), against Trajectory::evaluate and Trajectory::computeMinMaxMagnitude
// called per trajectory, bit for bit.  "host" runs the host policy, "device" the kernels
// (ExecutionPolicy::kDevice) and the batch object's members.
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

static void same_extremum(const char* what, int b, const mtg_extremum& got, const mtg::Extremum& want) {
  if (bits(got.time) != bits(want.time) || bits(got.value) != bits(want.value) || got.segment != want.segment_idx)
    std::printf("%s of trajectory %d: (%.17g, %.17g, %d), want (%.17g, %.17g, %d)\n", what, b, got.time, got.value,
                got.segment, want.time, want.value, want.segment_idx), ++fails;
}

int main(int argc, char** argv) {
  const bool device = argc > 1 && !std::strcmp(argv[1], "device");
  mtg::setExecutionPolicy(device ? mtg::ExecutionPolicy::kDevice : mtg::ExecutionPolicy::kHost);
  constexpr int N = 10;
  const int B = 5, D = 3, M = 8, nd = 3;
  const std::vector<int32_t> seg = {3, 1, 4, 1, 3};
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> uc(-2.0, 2.0), ut(0.3, 2.5), u01(0.0, 1.0);
  std::vector<mtg::Trajectory> traj(B);
  std::vector<double> coeffs, times, tq((size_t)B * M);
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
    double acc = 0.0, vertex1 = 0.0;  // the accumulated times as Trajectory::evaluate forms them
    for (int i = 0; i < seg[b]; ++i) {
      acc += t[i];
      if (i == 0) vertex1 = acc;
    }
    double* q = &tq[(size_t)b * M];
    q[0] = 0.0;
    q[1] = vertex1;     // a vertex time (K = 1: the end time)
    q[2] = acc;         // the end time: the last segment at its end
    q[3] = acc + 0.5;   // beyond the end: zeros
    q[4] = std::nextafter(acc, 0.0);
    for (int m = 5; m < M; ++m) q[m] = acc * u01(rng);
  }
  std::vector<double> out((size_t)B * M * nd * D, -1.0), out2(out.size(), -1.0);
  std::vector<uint8_t> in_range((size_t)B * M, 7);
  std::vector<int32_t> status(B, -1);
  std::vector<mtg_extremum> mn(B), mx(B), mn2(B), mx2(B);
  const uint32_t mask = 0b101;
  mtg::evaluateAtRagged<N>(D, B, seg.data(), coeffs.data(), times.data(), tq.data(), M, M, 0, nd, out.data(),
                           in_range.data(), status.data());
  mtg::minMaxMagnitudeRagged<N>(D, B, seg.data(), coeffs.data(), times.data(), 1, mask, mn.data(), mx.data());
  if (device) {
    mtg::BatchPolynomialOptimization<N> opt(D, 7, 4);  // (its segment count is not used)
    opt.evaluateAtRagged(B, seg.data(), coeffs.data(), times.data(), tq.data(), M, M, 0, nd, out2.data());
    opt.minMaxMagnitudeRagged(B, seg.data(), coeffs.data(), times.data(), 1, mask, mn2.data(), mx2.data());
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
    mtg::Extremum wmin, wmax;
    if (!traj[b].computeMinMaxMagnitude(1, {0, 2}, &wmin, &wmax)) std::printf("computeMinMaxMagnitude(%d) failed\n", b), ++fails;
    same_extremum("minimum", b, mn[b], wmin);
    same_extremum("maximum", b, mx[b], wmax);
    if (device) {
      same_extremum("member minimum", b, mn2[b], wmin);
      same_extremum("member maximum", b, mx2[b], wmax);
    }
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
