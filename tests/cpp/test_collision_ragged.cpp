// test_collision_ragged.cpp -- the free coefficientsFromVerticesRagged<10>, vertexDerivativesRagged<10> and
// collisionCostRagged<10> of batch_polynomial_optimization.h on five trajectories of 3, 1, 4, 1 and 3
// segments in one CSR batch (no K-group is one run of it), against the uniform entries called per
// trajectory, bit for bit: "host" runs the host policy against the uniform host entries with batch 1,
// "device" the kernels (ExecutionPolicy::kDevice) and the batch object's members against the uniform
// members of an object of that trajectory's K.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mav_trajectory_generation/batch_polynomial_optimization.h"

namespace mtg = mav_trajectory_generation;

static int fails = 0;

static void same(const char* what, int b, const double* got, const double* want, size_t n) {
  if (std::memcmp(got, want, n * sizeof(double))) std::printf("%s of trajectory %d differs\n", what, b), ++fails;
}

int main(int argc, char** argv) {
  const bool device = argc > 1 && !std::strcmp(argv[1], "device");
  mtg::setExecutionPolicy(device ? mtg::ExecutionPolicy::kDevice : mtg::ExecutionPolicy::kHost);
  constexpr int N = 10, h = N / 2, D = 3;
  const int B = 5;
  const std::vector<int32_t> seg = {3, 1, 4, 1, 3};
  std::vector<int64_t> so(B + 1, 0);
  for (int b = 0; b < B; ++b) so[b + 1] = so[b] + seg[b];
  const size_t totS = (size_t)so[B], totV = totS + B;

  // a sphere of radius 1 in a 32^3 grid of 0.25 m cells around the origin
  const int G = 32;
  std::vector<float> dist((size_t)G * G * G);
  mtg_sdf_grid grid{};
  grid.nx = grid.ny = grid.nz = G;
  grid.origin[0] = grid.origin[1] = grid.origin[2] = -4.0;
  grid.resolution = 0.25;
  grid.oob_distance = 5.0;
  for (int x = 0; x < G; ++x)
    for (int y = 0; y < G; ++y)
      for (int z = 0; z < G; ++z) {
        const double px = -4.0 + (x + 0.5) * 0.25 - 0.3, py = -4.0 + (y + 0.5) * 0.25 + 0.2, pz = -4.0 + (z + 0.5) * 0.25 - 0.1;
        dist[((size_t)x * G + y) * G + z] = (float)(std::sqrt(px * px + py * py + pz * pz) - 1.0);
      }
  grid.distance = dist.data();
  mtg_collision_params prm{};
  prm.coll_check_time_increment = 0.1;
  prm.map_resolution = 0.2;
  prm.epsilon = 0.5;
  prm.robot_radius = 0.3;
  prm.coll_pot_multiplier = 10.0;
  for (int k = 0; k < 3; ++k) prm.min_bound[k] = -4.0, prm.max_bound[k] = 4.0;
  prm.use_continuous_distance = 1;

  // vertex values: positions across the sphere, small velocities, the ends fixed, interior positions fixed
  std::mt19937_64 rng(20241021);
  std::uniform_real_distribution<double> up(-2.5, 2.5), uv(-0.5, 0.5), ut(1.0, 2.5);
  std::vector<double> x0(totV * h * D, 0.0), times(totS);
  std::vector<uint8_t> mask(totV);
  for (int b = 0; b < B; ++b)
    for (int v = 0; v <= seg[b]; ++v) {
      const size_t row = (size_t)so[b] + b + v;
      for (int d = 0; d < D; ++d) {
        x0[(row * h + 0) * D + d] = up(rng);
        x0[(row * h + 1) * D + d] = uv(rng);
      }
      mask[row] = (v == 0 || v == seg[b]) ? 31 : 1;
    }
  for (double& t : times) t = ut(rng);

  // values -> coeffs -> values (the coefficients are continuous, so the round trip stays close) -> collision
  std::vector<double> coeffs(totS * D * N, -1.0), x1(x0.size(), -1.0), cost(B, -1.0), grad(totV * h * D, -1.0);
  std::vector<uint8_t> coll(B, 7);
  std::vector<int32_t> nev(B, -1), status(B, -1);
  mtg::coefficientsFromVerticesRagged<N>(D, B, seg.data(), x0.data(), times.data(), coeffs.data());
  mtg::vertexDerivativesRagged<N>(D, B, seg.data(), coeffs.data(), times.data(), x1.data());
  mtg::collisionCostRagged<N>(B, seg.data(), x1.data(), mask.data(), times.data(), grid, prm, cost.data(), grad.data(),
                              coll.data(), nev.data(), status.data());
  std::vector<double> coeffs2(coeffs.size(), -2.0), x2(x0.size(), -2.0), cost2(B, -2.0), grad2(grad.size(), -2.0);
  std::vector<uint8_t> coll2(B, 9);
  std::vector<int32_t> nev2(B, -2), status2(B, -2);
  if (device) {
    mtg::BatchPolynomialOptimization<N> opt(D, 7, 4);  // (its segment count is not used)
    opt.coefficientsFromVerticesRagged(B, seg.data(), x0.data(), times.data(), coeffs2.data());
    opt.vertexDerivativesRagged(B, seg.data(), coeffs.data(), times.data(), x2.data());
    opt.collisionCostRagged(B, seg.data(), x1.data(), mask.data(), times.data(), grid, prm, cost2.data(), grad2.data(),
                            coll2.data(), nev2.data(), status2.data());
  }
  int evaluated = 0, costly = 0;
  for (int b = 0; b < B; ++b) {
    const int K = seg[b], V = K + 1;
    const size_t s0 = (size_t)so[b], v0 = s0 + b;
    std::vector<double> wc((size_t)K * D * N), wx((size_t)V * h * D), wg((size_t)D * V * h);
    double wcost = 0.0;
    uint8_t wcoll = 0;
    int32_t wnev = 0, wst = -1;
    if (device) {
      mtg::BatchPolynomialOptimization<N> one(D, K, 4);
      one.coefficientsFromVertices(1, &x0[v0 * h * D], &times[s0], wc.data());
      one.vertexDerivatives(1, &coeffs[s0 * D * N], &times[s0], wx.data());
      one.collisionCost(1, &x1[v0 * h * D], &mask[v0], &times[s0], grid, prm, &wcost, wg.data(), &wcoll, &wnev, &wst);
    } else {
      mtg::check(mtg_host_coefficients_from_vertices_batch(N, D, K, 1, &x0[v0 * h * D], &times[s0], wc.data(), 1), nullptr,
                 "mtg_host_coefficients_from_vertices_batch");
      mtg::check(mtg_host_vertex_derivatives_batch(N, D, K, 1, &coeffs[s0 * D * N], &times[s0], wx.data(), 1), nullptr,
                 "mtg_host_vertex_derivatives_batch");
      mtg::collisionCost<N>(K, 1, &x1[v0 * h * D], &mask[v0], &times[s0], grid, prm, &wcost, wg.data(), &wcoll, &wnev, &wst);
    }
    same("coefficients", b, &coeffs[s0 * D * N], wc.data(), wc.size());
    same("vertex derivatives", b, &x1[v0 * h * D], wx.data(), wx.size());
    same("cost", b, &cost[b], &wcost, 1);
    same("gradient", b, &grad[v0 * h * D], wg.data(), wg.size());
    if (coll[b] != wcoll || nev[b] != wnev || status[b] != wst || wst != MTG_TRAJ_OK)
      std::printf("trajectory %d: flag %d count %d status %d, want %d %d %d\n", b, coll[b], nev[b], status[b], wcoll, wnev, wst), ++fails;
    if (device) {
      same("member coefficients", b, &coeffs2[s0 * D * N], wc.data(), wc.size());
      same("member vertex derivatives", b, &x2[v0 * h * D], wx.data(), wx.size());
      same("member cost", b, &cost2[b], &wcost, 1);
      same("member gradient", b, &grad2[v0 * h * D], wg.data(), wg.size());
      if (coll2[b] != wcoll || nev2[b] != wnev || status2[b] != wst) std::printf("member: trajectory %d outputs differ\n", b), ++fails;
    }
    // the round trip moved no vertex value by more than rounding
    for (size_t i = 0; i < wx.size(); ++i)
      if (std::fabs(x1[v0 * h * D + i] - x0[v0 * h * D + i]) > 1e-9) std::printf("round trip: trajectory %d entry %zu\n", b, i), ++fails;
    evaluated += wnev;
    if (wcost > 0.0) ++costly;
  }
  if (evaluated < 50 || costly < 2)
    std::printf("only %d samples reached the potential, %d trajectories with a cost\n", evaluated, costly), ++fails;
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
