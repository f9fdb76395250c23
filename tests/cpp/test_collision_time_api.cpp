// test_collision_time_api.cpp -- collisionTimeGradient<N> of batch_polynomial_optimization.h against
// a hand-computed answer: a straight, constant-velocity flight parallel to a planar distance field
// (distance = z), whose polynomials continue as the same line past a segment's end.  "host" runs the
// host policy, "device" the kernel (ExecutionPolicy::kDevice) and the batch object's members.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"

namespace mtg = mav_trajectory_generation;

static int fails = 0;

static void near(const char* what, double got, double want) {
  if (!(std::fabs(got - want) <= 1e-12 * std::fabs(want))) std::printf("%s: %.17g, want %.17g\n", what, got, want), ++fails;
}
static void same(const char* what, long got, long want) {
  if (got != want) std::printf("%s: %ld, want %ld\n", what, got, want), ++fails;
}

int main(int argc, char** argv) {
  const bool device = argc > 1 && !std::strcmp(argv[1], "device");
  mtg::setExecutionPolicy(device ? mtg::ExecutionPolicy::kDevice : mtg::ExecutionPolicy::kHost);
  // planar field distance = z on a 64^3 grid, origin -8, resolution 0.25 (cell centres exact in float)
  const int n = 64;
  std::vector<float> field((size_t)n * n * n);
  for (int ix = 0; ix < n; ++ix)
    for (int iy = 0; iy < n; ++iy)
      for (int iz = 0; iz < n; ++iz) field[((size_t)ix * n + iy) * n + iz] = (float)(-8.0 + (iz + 0.5) * 0.25);
  mtg_sdf_grid grid{field.data(), n, n, n, {-8.0, -8.0, -8.0}, 0.25, 100.0};
  mtg_collision_params p{};
  p.coll_check_time_increment = 0.125;
  p.map_resolution = 0.0;  // every sample after the first reaches the potential
  p.epsilon = 0.5;
  p.robot_radius = 0.125;
  p.coll_pot_multiplier = 1.0;
  for (int k = 0; k < 3; ++k) p.min_bound[k] = -8.0, p.max_bound[k] = 8.0;
  p.use_continuous_distance = 0;

  // two segments, N = 6, x = -1 + 2 t along x at y = 0.125, z = 0.375: T = (1, 0.0625)
  const int K = 2, h = 3;
  const double v = 2.0, z0 = 0.375, dt = 0.125, inc = 0.25;
  const double T[2] = {1.0, 0.0625};
  const double xs[3] = {-1.0, 1.0, 1.125};
  std::vector<double> x((size_t)(K + 1) * h * 3, 0.0);
  for (int q = 0; q <= K; ++q) {
    x[(q * h + 0) * 3 + 0] = xs[q];
    x[(q * h + 0) * 3 + 1] = 0.125;
    x[(q * h + 0) * 3 + 2] = z0;
    x[(q * h + 1) * 3 + 0] = v;
  }
  // by hand.  d = z0 - radius = 0.25 <= epsilon: c = 0.5 / 0.5 * (0.25 - 0.5)^2 = 0.0625; every evaluated
  // sample adds c v dt.  After a segment whose clock ends exactly on its end time, time_sum is -dt, so the
  // first sample of segment 1 takes the first-entry branch and adds nothing.
  //   n = 0, smaller: T' = 0.75: samples t = 0 .. 0.625, five evaluated; bigger: T' = 1.25: nine
  //   n = 1: T <= 0.1, both sides 0.1: segment 0 gives seven, segment 1's only sample is a first entry
  const double term = 0.0625 * v * dt;
  double grad[2] = {-1.0, -1.0}, side[4] = {-1.0, -1.0, -1.0, -1.0};
  int32_t evaluated[4] = {-1, -1, -1, -1}, status = -1;
  mtg::collisionTimeGradient<6>(K, 1, x.data(), T, grid, p, grad, inc, side, evaluated, &status);
  same("status", status, MTG_TRAJ_OK);
  near("J(0, smaller)", side[0], 5.0 * term);
  near("J(0, bigger)", side[1], 9.0 * term);
  near("grad_t[0]", grad[0], 4.0 * term / (2.0 * inc));
  near("J(1, smaller)", side[2], 7.0 * term);
  near("J(1, bigger)", side[3], 7.0 * term);
  if (grad[1] != 0.0 || std::signbit(grad[1])) std::printf("grad_t[1]: %.17g, want +0.0\n", grad[1]), ++fails;
  const int32_t want_eval[4] = {5, 9, 7, 7};
  for (int q = 0; q < 4; ++q) same("side_evaluated", evaluated[q], want_eval[q]);

  // T[0] in (0.1, inc]: the reference CHECK-fails; NaN for that segment only
  const double T2[2] = {0.25, 0.0625};
  mtg::collisionTimeGradient<6>(K, 1, x.data(), T2, grid, p, grad, inc, side, evaluated, &status);
  same("status (NaN rule)", status, MTG_TRAJ_OK);
  if (!std::isnan(grad[0]) || !std::isnan(side[0]) || !std::isnan(side[1]) || evaluated[0] != 0 || evaluated[1] != 0)
    std::printf("T - inc <= 0 did not give NaN and zero counts for its segment\n"), ++fails;
  if (grad[1] != 0.0 || std::isnan(side[2])) std::printf("the NaN rule touched another segment\n"), ++fails;
  // a non-positive time: BAD_TIME, everything NaN
  const double T3[2] = {1.0, 0.0};
  mtg::collisionTimeGradient<6>(K, 1, x.data(), T3, grid, p, grad, inc, side, evaluated, &status);
  same("status (bad time)", status, MTG_TRAJ_BAD_TIME);
  if (!std::isnan(grad[0]) || !std::isnan(grad[1]) || !std::isnan(side[3]) || evaluated[2] != 0)
    std::printf("a bad time did not give NaN outputs\n"), ++fails;

  if (device) {  // the batch object: the kernel's diagnostic and the composed getCostAndGradientTime
    mtg::BatchPolynomialOptimization<6> opt(3, K, 2);
    double g2[2], s2[4];
    int32_t e2[4], walked = -1;
    opt.collisionTimeGradient(1, x.data(), T, grid, p, g2, inc, s2, e2, &walked, &status);
    mtg::collisionTimeGradient<6>(K, 1, x.data(), T, grid, p, grad, inc, side, evaluated, &status);
    if (std::memcmp(g2, grad, sizeof g2) || std::memcmp(s2, side, sizeof s2) || std::memcmp(e2, evaluated, sizeof e2))
      std::printf("member and free function differ\n"), ++fails;
    same("segments_walked", walked, 4 * K - 2);  // n = 0 walks segments 0 and 1, n = 1 its own
    double Jt = 0.0, gt[2], jd[2], jc[2], cost = 0.0, jac[2];
    const double ones[2] = {1.0, 1.0};
    opt.timeGradient(1, x.data(), T, grid, p, 0.1, 10.0, 1.0, &Jt, gt, inc, jd, jc);
    opt.timeJacobian(1, x.data(), T, 1, ones, &cost, jac, inc);
    near("J_t", Jt, 1.0625);
    if (std::memcmp(jd, jac, sizeof jd) || std::memcmp(jc, grad, sizeof jc)) std::printf("timeGradient's parts differ\n"), ++fails;
    for (int i = 0; i < K; ++i)
      if (gt[i] != (0.1 * jd[i] + 10.0 * jc[i]) + 1.0) std::printf("timeGradient[%d] is not the stated sum\n", i), ++fails;
  }

#ifdef MTG_CPP_THROW
  const double bad_inc[3] = {0.0, -0.1, INFINITY};
  for (double bi : bad_inc) {
    bool threw = false;
    try {
      mtg::collisionTimeGradient<6>(K, 1, x.data(), T, grid, p, grad, bi);
    } catch (const mtg::Error& e) {
      threw = e.code == MTG_ERR_INVALID_ARGUMENT;
    }
    if (!threw) std::printf("increment_time = %g did not raise MTG_ERR_INVALID_ARGUMENT\n", bi), ++fails;
  }
#endif
  if (fails) return 1;
  std::printf("all checks passed\n");
  return 0;
}
