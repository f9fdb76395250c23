// test_segment_extrema.cpp -- the per-segment extremum layer of the C++ drop-in:
// Polynomial::computeMinMaxCandidates / computeMinMax / selectMinMaxFromCandidates and
// Segment::computeMinMaxMagnitudeCandidateTimes / computeMinMaxMagnitudeCandidates /
// selectMinMaxMagnitudeFromCandidates, plus the free segmentMinMaxMagnitude<N> / segmentMinMaxAxis<N>.
// The first block is the loop of the reference's extremum test
// (test/test_polynomial_optimization.cpp:441-490) against these headers.  "host" runs the host policy,
// "device" sends the Segment methods and the free functions through the kernels.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"
#include "mav_trajectory_generation/polynomial_optimization_linear.h"
#include "mav_trajectory_generation/trajectory.h"

using namespace mav_trajectory_generation;

static int fails = 0;
#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      std::printf("FAILED %s: ", #cond);         \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
      ++fails;                                   \
    }                                            \
  } while (0)

// Root times of the two root routines (this layer's and computeSegmentMaximumMagnitudeCandidates')
// agree to the tolerance tests/test_segment_extrema_host.py measures on its constructed fixture and
// allows the device (10 x 2.3e-12 of the window), relative to the segment time.
static constexpr double kRootTimeTol = 2.3e-11;

static VectorXd vec(std::initializer_list<double> v) {
  VectorXd out((int)v.size());
  int i = 0;
  for (double x : v) out[i++] = x;
  return out;
}

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol * std::fmax(1.0, std::fabs(b)); }

int main(int argc, char** argv) {
  const bool device = argc > 1 && !std::strcmp(argv[1], "device");
  setExecutionPolicy(device ? ExecutionPolicy::kDevice : ExecutionPolicy::kHost);
  constexpr int N = 10;

  // ---- the reference's loop: one dimension, velocity
  for (unsigned seed : {12345u, 7u, 99u}) {
    Vertex::Vector vertices = createRandomVertices(derivative_order::SNAP, 6, vec({-10.0}), vec({10.0}), seed);
    const std::vector<double> times = estimateSegmentTimes(vertices, 3.0, 5.0);
    PolynomialOptimization<N> opt(1);
    opt.setupFromVertices(vertices, times, derivative_order::SNAP);
    opt.solveLinear();
    Segment::Vector segments;
    opt.getSegments(&segments);
    int idx = 0;
    for (const Segment& s : segments) {
      std::vector<double> res, res_template_free;
      opt.computeSegmentMaximumMagnitudeCandidates<1>(s, 0, s.getTime(), &res);
      const bool ok = s.computeMinMaxMagnitudeCandidateTimes(1, 0.0, s.getTime(), {0}, &res_template_free);
      EXPECT(ok, "computeMinMaxMagnitudeCandidateTimes returned false (seed %u segment %d)", seed, idx);
      EXPECT(res_template_free.size() >= 2 && res_template_free[0] == 0.0 && res_template_free[1] == s.getTime(),
             "the ends come first (seed %u segment %d)", seed, idx);
      EXPECT(res.size() + 2 == res_template_free.size(), "seed %u segment %d: %zu roots against %zu", seed, idx,
             res.size(), res_template_free.size() - 2);
      for (size_t i = 0; i < res.size() && i + 2 < res_template_free.size(); ++i)
        EXPECT(std::fabs(res[i] - res_template_free[i + 2]) <= kRootTimeTol * s.getTime(),
               "seed %u segment %d root %zu: %.17g against %.17g", seed, idx, i, res_template_free[i + 2], res[i]);
      ++idx;
    }
  }

  // ---- three dimensions: candidates + selection reproduce Trajectory::computeMinMaxMagnitude per segment
  {
    Vertex::Vector vertices =
        createRandomVertices(derivative_order::SNAP, 4, vec({-10.0, -20.0, -10.0}), vec({10.0, 20.0, 10.0}), 4242);
    const std::vector<double> times = estimateSegmentTimes(vertices, 3.0, 5.0);
    PolynomialOptimization<N> opt(3);
    opt.setupFromVertices(vertices, times, derivative_order::SNAP);
    opt.solveLinear();
    Segment::Vector segments;
    opt.getSegments(&segments);
    const std::vector<int> dims = {0, 1, 2};
    std::vector<double> coeffs, seg_times;
    for (const Segment& s : segments) {
      std::vector<Extremum> cand;
      EXPECT(s.computeMinMaxMagnitudeCandidates(2, 0.0, s.getTime(), dims, &cand), "computeMinMaxMagnitudeCandidates");
      Extremum mn, mx, wmn, wmx;
      EXPECT(s.selectMinMaxMagnitudeFromCandidates(0.0, s.getTime(), 2, dims, cand, &mn, &mx), "select");
      Trajectory one;
      one.setSegments(Segment::Vector(1, s));
      EXPECT(one.computeMinMaxMagnitude(2, dims, &wmn, &wmx), "computeMinMaxMagnitude");
      EXPECT(near(mn.value, wmn.value, 1e-11) && near(mx.value, wmx.value, 1e-11),
             "segment extremes (%.17g, %.17g) against the trajectory's (%.17g, %.17g)", mn.value, mx.value, wmn.value,
             wmx.value);
      EXPECT(mn.segment_idx == 0 && mx.segment_idx == 0, "segment index stays 0");
      std::vector<double> c, t;
      one.pack(&c, &t);
      coeffs.insert(coeffs.end(), c.begin(), c.end());
      seg_times.push_back(t[0]);
    }
    // the free functions on the same segments: the magnitude entry equals the per-segment trajectory result bit
    // for bit on [0, T]; the axis entry brackets the sampled signed values
    const int S = (int)segments.size();
    std::vector<mtg_extremum> mn(S), mx(S), amn((size_t)S * 3), amx((size_t)S * 3);
    std::vector<int32_t> count(S), status(S);
    segmentMinMaxMagnitude<N>(3, S, coeffs.data(), seg_times.data(), nullptr, 2, 0, mn.data(), mx.data(), nullptr,
                              count.data(), 0, status.data());
    segmentMinMaxAxis<N>(3, S, coeffs.data(), seg_times.data(), nullptr, 2, amn.data(), amx.data());
    for (int i = 0; i < S; ++i) {
      Trajectory one;
      one.setSegments(Segment::Vector(1, segments[(size_t)i]));
      Extremum wmn, wmx;
      one.computeMinMaxMagnitude(2, dims, &wmn, &wmx);
      EXPECT(status[i] == MTG_TRAJ_OK && count[i] >= 2, "status / count of segment %d", i);
      EXPECT(mn[i].time == wmn.time && mn[i].value == wmn.value && mx[i].time == wmx.time && mx[i].value == wmx.value,
             "segmentMinMaxMagnitude of segment %d differs from the trajectory entry", i);
      for (int d = 0; d < 3; ++d)
        for (int q = 0; q <= 50; ++q) {
          const double t = seg_times[i] * q / 50.0, v = segments[(size_t)i][(size_t)d].evaluate(t, 2);
          const double slack = 1e-9 * std::fmax(std::fabs(amn[(size_t)i * 3 + d].value), std::fabs(amx[(size_t)i * 3 + d].value));
          EXPECT(v >= amn[(size_t)i * 3 + d].value - slack && v <= amx[(size_t)i * 3 + d].value + slack,
                 "axis range of segment %d dimension %d does not hold %.17g at %.17g", i, d, v, t);
        }
    }
  }

  // ---- Polynomial::computeMinMax on known polynomials
  {
    const Polynomial p(4, vec({0.0, -3.0, 0.0, 1.0}));  // t^3 - 3 t: p' = 3 (t - 1)(t + 1)
    std::vector<double> cand;
    EXPECT(p.computeMinMaxCandidates(-2.0, 2.0, 0, &cand), "candidates of the cubic");
    // (-1 and 1 are sample points of [-2, 2]: exact zeros of p', found exactly)
    EXPECT(cand.size() == 4 && cand[0] == -2.0 && cand[1] == 2.0 && cand[2] == -1.0 && cand[3] == 1.0,
           "cubic candidates: %zu", cand.size());
    std::pair<double, double> mn, mx, smn, smx;
    EXPECT(p.computeMinMax(-2.0, 2.0, 0, &mn, &mx), "computeMinMax");
    // p(-2) = p(1) = -2 and p(2) = p(-1) = 2: the first candidate wins both ties
    EXPECT(mn.first == -2.0 && mn.second == -2.0 && mx.first == 2.0 && mx.second == 2.0,
           "cubic extremes (%g, %g) (%g, %g)", mn.first, mn.second, mx.first, mx.second);
    EXPECT(p.selectMinMaxFromCandidates(cand, 0, &smn, &smx) && smn == mn && smx == mx, "selectMinMaxFromCandidates");
    EXPECT(p.computeMinMax(0.0, 3.0, 0, &mn, &mx), "computeMinMax on [0, 3]");
    EXPECT(near(mn.first, 1.0, 1e-12) && near(mn.second, -2.0, 1e-12) && mx.first == 3.0 && mx.second == 18.0,
           "cubic on [0, 3]: (%.17g, %.17g) (%.17g, %.17g)", mn.first, mn.second, mx.first, mx.second);
    EXPECT(p.computeMinMax(0.0, 3.0, 1, &mn, &mx), "velocity of the cubic");  // 3 t^2 - 3: root of p'' at 0 = t_start
    EXPECT(mn.first == 0.0 && mn.second == -3.0 && mx.first == 3.0 && mx.second == 24.0, "cubic velocity extremes");
    const Polynomial q(5, vec({0.0, 0.0, -2.0, 0.0, 1.0}));  // odd N: t^4 - 2 t^2, q' = 4 t (t - 1)(t + 1)
    EXPECT(q.computeMinMaxCandidates(-0.5, 2.0, 0, &cand), "candidates of the quartic");
    EXPECT(cand.size() == 4 && near(cand[2], 0.0, 1e-12) && std::fabs(cand[2]) < 1e-12 && near(cand[3], 1.0, 1e-12),
           "quartic candidates: %zu", cand.size());
    const Polynomial z(6);  // the zero polynomial: no roots (rpoly.cpp:62-65), the two ends
    EXPECT(z.computeMinMaxCandidates(0.0, 1.0, 0, &cand) && cand.size() == 2, "zero polynomial: %zu candidates", cand.size());
    EXPECT(z.computeMinMax(0.0, 1.0, 0, &mn, &mx) && mn.first == 0.0 && mx.first == 0.0 && mn.second == 0.0,
           "zero polynomial extremes");
    // the false returns
    EXPECT(!p.computeMinMax(1.0, 0.0, 0, &mn, &mx), "t_start > t_end");
    EXPECT(!p.computeMinMaxCandidates(1.0, 0.0, 0, &cand) && cand.empty(), "t_start > t_end (candidates)");
    EXPECT(!p.computeMinMaxCandidates(0.0, 1.0, 4, &cand), "N - derivative - 1 < 0");
    EXPECT(!p.selectMinMaxFromCandidates({}, 0, &mn, &mx), "empty candidates");
  }
  {
    Segment s(N, 2);
    s.setTime(1.5);
    s[0].setCoefficients(vec({1.0, -2.0, 0.5, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}));
    s[1].setCoefficients(vec({0.0, 1.0, -1.0, 0.0, 0.125, 0.0, 0.0, 0.0, 0.0, 0.0}));
    std::vector<double> t;
    std::vector<Extremum> cand;
    Extremum mn, mx;
    EXPECT(!s.computeMinMaxMagnitudeCandidateTimes(1, 0.0, 1.5, {}, &t), "no dimensions");
    EXPECT(!s.computeMinMaxMagnitudeCandidateTimes(1, 0.0, 1.5, {0, 2}, &t), "dimension out of range");
    EXPECT(!s.computeMinMaxMagnitudeCandidateTimes(1, 1.5, 0.0, {0, 1}, &t) && t.empty(), "t_start > t_end");
    EXPECT(!s.selectMinMaxMagnitudeFromCandidates(1.5, 0.0, 1, {0, 1}, cand, &mn, &mx), "select: t_start > t_end");
    // a window inside the segment: candidates outside it are skipped by the selection
    EXPECT(s.computeMinMaxMagnitudeCandidates(0, 0.0, 1.5, {0, 1}, &cand) && cand.size() >= 2, "candidates");
    EXPECT(s.selectMinMaxMagnitudeFromCandidates(0.25, 0.5, 0, {0, 1}, cand, &mn, &mx), "select on a sub-window");
    EXPECT(mn.time >= 0.25 && mn.time <= 0.5 && mx.time >= 0.25 && mx.time <= 0.5, "selected times in the window");
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
